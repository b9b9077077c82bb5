// fits_rules.h -- what the FITS image unpacker decides (fitsin.hip), each rule stated once over plain values: which BITPIX it takes,
// the window check, the choice between the 16-byte vector path and the scalar path of a row (head, body, tail), the float64 ->
// float32 conversion on bit patterns, the carry fold of the DATASUM word sum, and the launch sizes.  No device code, no HIP runtime:
// the kernels call these from their parallel plumbing, tests/hostsim/fits_rules_host.cpp calls them serially under AddressSanitizer
// and UBSan, and tests/test_ffi_host.py holds that to Python and numpy.
#pragma once
#include <cstdint>

#ifndef TP_RULE
#if defined(__HIPCC__)
#define TP_RULE __host__ __device__
#else
#define TP_RULE
#endif
#endif

namespace tp_fits {

constexpr int kThreads = 256;          // every block
constexpr int kSumBlocks = 2048;       // at most this many blocks add up a data unit (8 per CU)
constexpr int kSumUnroll = 4;          // 16-byte loads a thread has in flight
constexpr int64_t kMaxAxis = 1 << 24;  // NAXIS1, NAXIS2: their product times 8 stays far inside int64
constexpr uint64_t kMaxSumBytes = (uint64_t)1 << 34;   // fewer than 2^32 words: their 64-bit sum cannot wrap

// bytes per pixel of the BITPIX values the unpacker takes (IEEE float images), 0 for every other
TP_RULE inline int item_bytes(int32_t bitpix) { return bitpix == -32 ? 4 : bitpix == -64 ? 8 : 0; }

TP_RULE inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// the message of the first rule a call breaks, or null.  Addresses travel as integers.
inline const char* unpack_check(uint64_t raw_addr, int32_t bitpix, int64_t naxis1, int64_t naxis2, int64_t row0, int64_t col0, int64_t rows, int64_t cols,
	uint64_t out_addr, int64_t out_row_pitch)
{
	if (item_bytes(bitpix) == 0) return "tp_fits_unpack: BITPIX must be -32 or -64 (integer images are not supported)";
	if (!(naxis1 >= 1 && naxis2 >= 1 && naxis1 <= kMaxAxis && naxis2 <= kMaxAxis)) return "tp_fits_unpack: NAXIS1 and NAXIS2 must lie in [1, 2^24]";
	if (!(rows >= 1 && cols >= 1)) return "tp_fits_unpack: the window must have at least one row and one column";
	if (!(row0 >= 0 && col0 >= 0 && rows <= naxis2 - row0 && cols <= naxis1 - col0)) return "tp_fits_unpack: the window leaves the image";
	if (!(out_row_pitch >= cols)) return "tp_fits_unpack: out_row_pitch below the window's columns";
	if (raw_addr == 0 || out_addr == 0) return "tp_fits_unpack: null pointer";
	if (raw_addr % 16 != 0) return "tp_fits_unpack: d_raw must be 16-byte aligned";
	if (out_addr % 4 != 0) return "tp_fits_unpack: d_out must be 4-byte aligned";
	return nullptr;
}

// How the rows of a window are moved.  vec = 1: every row is `head` single values, then `body4` groups of four values that start on a
// 16-byte boundary in the file and in the output alike, then `tail` single values.  vec = 0: single values only (head = cols).
// The vector path needs the same boundaries in every row: a row of the file and a row of the output are multiples of 16 bytes, and
// where the output reaches a boundary (after `head` values) the file is on one too.  The TESS science window is all body:
// col0 = 44 is 176 bytes into rows of 8544 bytes, 2048 columns are 512 groups.
struct RowPlan {
	int32_t vec;
	int64_t head, body4, tail;
};
TP_RULE inline RowPlan row_plan(uint64_t raw_addr, int item, int64_t naxis1, int64_t row0, int64_t col0, int64_t cols, uint64_t out_addr, int64_t out_row_pitch)
{
	RowPlan p{0, cols, 0, 0};
	if ((naxis1 * item) % 16 != 0 || out_row_pitch % 4 != 0) return p;
	const int64_t head = (int64_t)((4 - (out_addr / 4) % 4) % 4);                        // values until the output is on a boundary
	const uint64_t src = raw_addr + (uint64_t)((row0 * naxis1 + col0 + head) * item);      // the file there
	if (src % 16 != 0 || cols - head < 4) return p;
	p.vec = 1;
	p.head = head;
	p.body4 = (cols - head) / 4;
	p.tail = (cols - head) % 4;
	return p;
}

// float64 -> float32 on the bit patterns, round to nearest even, as a C cast / numpy's astype('float32') gives on the host: the
// result may be a denormal (nothing is flushed to zero) or infinite; a NaN keeps its sign and the top 22 bits of its payload and
// comes back quiet.
TP_RULE inline uint32_t f64_to_f32_bits(uint64_t u)
{
	const uint32_t sign = (uint32_t)(u >> 63) << 31;
	const int32_t e = (int32_t)((u >> 52) & 0x7ff);
	const uint64_t m = u & 0xfffffffffffffull;
	if (e == 0x7ff) return m ? (sign | 0x7fc00000u | (uint32_t)(m >> 29)) : (sign | 0x7f800000u);
	if (e == 0) return sign;                            // zero and the float64 denormals: far below half the smallest float32
	const int32_t ef = e - 1023 + 127;
	if (ef >= 255) return sign | 0x7f800000u;
	uint64_t sig, rem, half;
	uint32_t r;
	if (ef >= 1) {
		sig = m >> 29;
		rem = m & 0x1fffffffull;
		half = 0x10000000ull;
		r = sign | ((uint32_t)ef << 23) | (uint32_t)sig;
	} else {
		const int shift = 30 - ef;                        // the 53-bit significand in units of 2^-149
		if (shift > 54) return sign;                      // below a quarter of the unit
		const uint64_t full = m | 0x10000000000000ull;
		sig = full >> shift;
		rem = full & (((uint64_t)1 << shift) - 1);
		half = (uint64_t)1 << (shift - 1);
		r = sign | (uint32_t)sig;
	}
	if (rem > half || (rem == half && (sig & 1))) r++;   // a carry out of the mantissa raises the exponent: up to infinity, or to the smallest normal
	return r;
}

// DATASUM: the ones'-complement sum of 32-bit words from their plain 64-bit sum (the carries folded back in at the end)
TP_RULE inline uint64_t fold32(uint64_t s)
{
	while (s >> 32) s = (s & 0xffffffffull) + (s >> 32);
	return s;
}

inline const char* datasum_check(uint64_t raw_addr, uint64_t nbytes, uint64_t sum_addr)
{
	if (nbytes % 4 != 0) return "tp_fits_datasum: the byte count must be a multiple of 4";
	if (nbytes >= kMaxSumBytes) return "tp_fits_datasum: a data unit holds fewer than 2^34 bytes";
	if (sum_addr == 0 || (nbytes && raw_addr == 0)) return "tp_fits_datasum: null pointer";
	if (raw_addr % 16 != 0) return "tp_fits_datasum: d_raw must be 16-byte aligned";
	if (sum_addr % 8 != 0) return "tp_fits_datasum: d_wordsum must be 8-byte aligned";
	return nullptr;
}
// blocks that add up n16 pieces of 16 bytes: one per kThreads * kSumUnroll pieces, at least 1, at most kSumBlocks
inline int64_t sum_blocks(uint64_t n16)
{
	const uint64_t per = (uint64_t)kThreads * kSumUnroll;
	const uint64_t b = (n16 + per - 1) / per;
	return (int64_t)(b < 1 ? 1 : b > (uint64_t)kSumBlocks ? (uint64_t)kSumBlocks : b);
}

} // namespace tp_fits
