// select_rules.h -- selection by rank without a sort, the rules stated once over plain values: the order-preserving keys of float64 /
// float32 values and the bookkeeping of an MSB-first radix pass.  No device code, no HIP runtime: Halo photometry (halo_rules.h,
// halo_dev.h) and the radial background (radial_rules.h, radial.hip) call these from their parallel plumbing; the host drivers under
// tests/hostsim compose them serially under AddressSanitizer and UBSan.
// (diagnostics.hip keeps the one remaining copy of the float64 key, sort_key, beside its block_median.)
#pragma once
#include <cstdint>

#ifndef TP_RULE
#if defined(__HIPCC__)
#define TP_RULE __host__ __device__
#else
#define TP_RULE
#endif
#endif

namespace tp_select {

//--------------------------------------------------------------------------------------------------
// keys: unsigned integers in the order of the values (-inf < ... < -0 < +0 < ... < +inf), and back
//--------------------------------------------------------------------------------------------------
TP_RULE inline uint64_t okey(double v)
{
	const uint64_t u = __builtin_bit_cast(uint64_t, v);
	return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
TP_RULE inline double from_key(uint64_t k) { return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }
TP_RULE inline uint32_t fkey(float v)
{
	const uint32_t u = __builtin_bit_cast(uint32_t, v);
	return (u >> 31) ? ~u : (u | 0x80000000u);
}
TP_RULE inline float from_fkey(uint32_t k) { return __builtin_bit_cast(float, (k >> 31) ? (k & 0x7fffffffu) : ~k); }

// Radix selection of the key of rank k, most significant byte first: a pass counts the digit at `shift` of the keys that agree with
// `prefix` on the bytes above (`mask`); the bin that holds the rank becomes the next byte of the prefix, the rank goes on as the
// remainder inside the bin.  After the last pass the prefix is the key and `krem` counts the equal keys before the selected one.
struct RadixPass {
	uint64_t prefix, mask;
	int shift, krem;
};
TP_RULE inline RadixPass radix_begin(int k) { return RadixPass{0, 0, 56, k}; }
TP_RULE inline bool radix_takes_part(const RadixPass& p, uint64_t key) { return (key & p.mask) == p.prefix; }
TP_RULE inline int radix_digit(const RadixPass& p, uint64_t key) { return (int)((key >> p.shift) & 255); }
// bins c[0 .. n) starting at number b with `cum` keys below them: on to the bin that holds rank krem (the last one takes the rest)
TP_RULE inline void radix_walk(const int* c, int n, int krem, int& b, int& cum)
{
	for (int i = 0; i + 1 < n && krem >= cum + c[i]; i++) {
		cum += c[i];
		b++;
	}
}
// false after the last pass
TP_RULE inline bool radix_next(RadixPass& p, int bin, int rem)
{
	p.prefix |= (uint64_t)bin << p.shift;
	p.mask |= (uint64_t)255 << p.shift;
	p.krem = rem;
	p.shift -= 8;
	return p.shift >= 0;
}

} // namespace tp_select
