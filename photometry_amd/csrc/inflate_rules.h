// inflate_rules.h -- what the batched DEFLATE decoder decides (inflate.hip; RFC 1951), each rule stated once over plain values: the bit
// reader, the block headers, the code-length code with its repeat symbols, the canonical decoding tables, the literal / length /
// distance decode, the window copy, the flush of finished bytes with their CRC-32, the statuses, and the refusals of tp_inflate.  Every
// index the decoder forms is formed here.  The tables of lengths and distances, cl_order and the CRC functions are deflate_rules.h's.
//
// One wavefront owns a stream; its state is the struct Lds below (39.6 KiB: four streams per CU).  The chain of symbols is serial
// and the same on every lane (wave-uniform: what comes out of LDS goes through TP_INFLATE_UNIFORM).  The lanes share the work of
//   the input refill   aligned words of the stream into Lds::stage (bytes outside the stream read as zero and are never loaded)
//   the table build    counts per length, symbols sorted by (length, symbol), the fast tables
//   the stored copy    and the runs of the code-length symbols 16, 17, 18
//   the match copy     rows of 64 bytes, element k from start + k % dist, a row read before it is written
//   the flush          finished window bytes to memory in aligned words, their CRC from 64 slices (crc_slice_term, crc_combine)
// Such a piece is written once, as TP_INFLATE_LANES(lane) { ... }: in the kernel the wavefront's lanes run it side by side between
// two barriers, on the host the lanes run it one after the other -- tests/hostsim/inflate_rules_host.cpp calls the same
// inflate_stream under AddressSanitizer and UBSan with buffers of exactly the sizes a call may touch.
//
// The window is a ring of 32 KiB in LDS, indexed by the low bits of the byte's address in memory, so that aligned words of memory are
// aligned words of the ring.  A match reads bytes that other lanes stored an instruction earlier: LDS operations of a wavefront
// complete in order.  Bytes leave the ring when it is about to be overwritten (room) and at the end, never past the bytes produced.
//
// Acceptance is zlib's (inflate.c, inftrees.c):
//   HLIT > 286 or HDIST > 30 is refused (TOO_MANY_SYMBOLS)
//   symbol 16 with no previous length, and a repeat that runs past HLIT + HDIST, are refused (BAD_CODE_LENGTHS)
//   an over-subscribed code is refused (BAD_CODE_LENGTHS)
//   an incomplete code is refused (BAD_CODE_LENGTHS), except a literal/length or distance code whose longest code is 1 bit
//   a literal/length or distance code with no symbol at all is taken and fails when it is used (BAD_SYMBOL); a code-length code
//     with no symbol is refused here: zlib reads every length as 0 from it and then misses the end-of-block code
//   len[256] == 0 is refused (NO_END_OF_BLOCK)
//   a distance larger than the bytes produced so far is refused (DISTANCE_TOO_FAR)
//   the length symbols 286 / 287 and the distance symbols 30 / 31 (fixed blocks) are refused (BAD_SYMBOL)
//   a bit that lies behind the stream's end is never taken (INPUT_ENDS); a byte that does not fit the slot is never written (OUTPUT_FULL)
// Every loop takes at least one bit of input or ends: a stream is over after at most 8 * input bytes steps, whatever it holds.
#pragma once
#include <cstdint>
#include "deflate_rules.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TP_INFLATE_UNIFORM(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))
#define TP_INFLATE_XOR(ref, v) atomicXor(&(ref), (v))
#define TP_INFLATE_SLOTS 1
#define TP_INFLATE_SLOT(lane) 0
// the lanes of the wavefront side by side, a barrier before and behind
#define TP_INFLATE_LANES(lane) __syncthreads(); for (int lane = (int)threadIdx.x, tp_once_ = 1; tp_once_; tp_once_ = 0, __syncthreads())
#define TP_INFLATE_ONE_LANE if (threadIdx.x == 0)
#else
#define TP_INFLATE_UNIFORM(v) ((uint32_t)(v))
#define TP_INFLATE_XOR(ref, v) do { (ref) ^= (v); } while (0)
#define TP_INFLATE_SLOTS 64
#define TP_INFLATE_SLOT(lane) (lane)
#define TP_INFLATE_LANES(lane) for (int lane = 0; lane < tp_inflate_rules::kLanes; lane++)
#define TP_INFLATE_ONE_LANE
#endif

namespace tp_inflate_rules {

using tp_deflate_rules::kLanes;
using tp_deflate_rules::kNumCL;
using tp_deflate_rules::kEob;
using tp_deflate_rules::kMaxTotal;

constexpr uint32_t kWindow = 32768;            // bytes of the ring: the largest distance
constexpr uint32_t kStageWords = 512;          // words of input in LDS between two refills
constexpr int kMaxBits = 15, kMaxBitsCL = 7;
constexpr int kFastBitsLL = 10, kFastBitsD = 8;   // codes up to these lengths are one table look-up
constexpr int kMaxLL = 288, kMaxD = 32;        // the fixed codes' alphabets
constexpr uint32_t kPiece = 4096;              // bytes of a stored block copied between two looks at the ring's room

enum Status : int32_t {
	kOk = 0, kInputEnds = 1, kBadBlockType = 2, kStoredLength = 3, kTooManySymbols = 4, kBadCodeLengths = 5, kNoEndOfBlock = 6, kBadSymbol = 7,
	kDistanceTooFar = 8, kOutputFull = 9
};
enum Kind { kCodes = 0, kLens = 1, kDists = 2 };

// one stream of a call: where its input lies in d_in, where its slot lies in d_out
struct StreamDesc {
	uint64_t in_begin, in_bytes, out_begin, out_capacity;
};

// the state of a stream: LDS in the kernel
struct Lds {
	uint32_t window[kWindow / 4];
	uint32_t stage[kStageWords];
	uint32_t crc_table[256];
	uint16_t fast_ll[1 << kFastBitsLL], fast_d[1 << kFastBitsD];   // symbol << 4 | code length, 0: not a code of the table's lengths
	uint16_t sym_ll[kMaxLL], sym_d[kMaxD], sym_cl[20];             // the symbols sorted by (code length, symbol)
	uint32_t count_ll[16], count_d[16], count_cl[16];              // symbols per code length
	uint8_t len[kMaxLL + kMaxD];                                   // the code lengths of a block, literal/length then distance
	uint8_t len_cl[20];
	uint32_t crc_acc;
};

// what a stream's wavefront carries in registers
struct State {
	const unsigned char* src;      // the stream [src, src + n)
	uint64_t n;
	uint32_t shift;                // address of src & 3
	uint64_t pos;                  // the next bit
	uint64_t w0;                   // the stage holds the words [w0, w0 + kStageWords) of the stream, moved up by `shift` bytes
	uint64_t hold, hold_pos;       // 64 bits of the stream from bit hold_pos (a byte's first), when hold_set
	bool hold_set;
	unsigned char* dst;            // the slot [dst, dst + capacity)
	uint64_t capacity;
	uint32_t oshift;               // address of dst & 3
	uint64_t out, flushed;         // bytes produced, bytes in memory
	uint32_t crc;                  // of the bytes in memory
};

struct Result {
	int32_t status;
	uint64_t out_bytes, in_bytes;
	uint32_t crc;
};

// ---- refusals of tp_inflate ---------------------------------------------------------------------------------------------------------
// the message of the first rule a call breaks, or null.  Addresses travel as integers; the offsets are host memory.
// Alignments: d_in and d_out none (bytes), d_status 4, d_out_bytes 8, d_in_bytes 8, d_crc 4.
inline const char* check(uint64_t in_addr, const uint64_t* in_offsets, int64_t n_streams, uint64_t out_addr, const uint64_t* out_offsets, uint64_t status_addr,
	uint64_t out_bytes_addr, uint64_t in_bytes_addr, uint64_t crc_addr)
{
	if (n_streams < 1) return "tp_inflate: n_streams must be at least 1";
	if (in_offsets == nullptr || out_offsets == nullptr) return "tp_inflate: null pointer";
	for (int64_t s = 0; s < n_streams; s++)
		if (in_offsets[s + 1] < in_offsets[s] || out_offsets[s + 1] < out_offsets[s]) return "tp_inflate: the stream offsets must not fall";
	if (in_offsets[n_streams] - in_offsets[0] >= kMaxTotal || in_offsets[n_streams] >= ((uint64_t)1 << 62)) return "tp_inflate: a call holds fewer than 2^34 bytes";
	if (out_offsets[n_streams] - out_offsets[0] >= kMaxTotal || out_offsets[n_streams] >= ((uint64_t)1 << 62)) return "tp_inflate: a call holds fewer than 2^34 bytes";
	if (status_addr == 0 || out_bytes_addr == 0 || in_bytes_addr == 0 || crc_addr == 0) return "tp_inflate: null pointer";
	if (in_addr == 0 && in_offsets[n_streams] != in_offsets[0]) return "tp_inflate: null pointer";
	if (out_addr == 0 && out_offsets[n_streams] != out_offsets[0]) return "tp_inflate: null pointer";
	if (status_addr % 4 != 0) return "tp_inflate: d_status must be 4-byte aligned";
	if (out_bytes_addr % 8 != 0) return "tp_inflate: d_out_bytes must be 8-byte aligned";
	if (in_bytes_addr % 8 != 0) return "tp_inflate: d_in_bytes must be 8-byte aligned";
	if (crc_addr % 4 != 0) return "tp_inflate: d_crc must be 4-byte aligned";
	return nullptr;
}

// the stream table of a call; `table` holds n_streams entries
inline void stream_table(const uint64_t* in_offsets, const uint64_t* out_offsets, int64_t n_streams, StreamDesc* table)
{
	for (int64_t s = 0; s < n_streams; s++)
		table[s] = StreamDesc{in_offsets[s], in_offsets[s + 1] - in_offsets[s], out_offsets[s], out_offsets[s + 1] - out_offsets[s]};
}

// ---- code tables --------------------------------------------------------------------------------------------------------------------
// the smallest length of symbol 257 .. 285 and the smallest distance of symbol 0 .. 29 (RFC 1951, 3.2.5); the extra bits are
// deflate_rules.h's length_extra_bits and distance_extra_bits
TP_RULE inline uint32_t length_base(int sym)
{
	if (sym == 285) return 258;
	if (sym < 265) return (uint32_t)(sym - 254);
	return 3u + ((4u + (uint32_t)((sym - 265) & 3)) << tp_deflate_rules::length_extra_bits(sym));
}
TP_RULE inline uint32_t distance_base(int sym)
{
	if (sym < 4) return (uint32_t)(sym + 1);
	return 1u + ((2u + (uint32_t)(sym & 1)) << tp_deflate_rules::distance_extra_bits(sym));
}

// Decode one symbol of a canonical code from `bits` (least significant first, max_len of them valid): the symbol and its length, or
// -1 when no code of up to max_len bits begins them.  count[l]: symbols of length l; symbol[]: the symbols by (length, symbol).
// For a code that is not over-subscribed the index stays below the number of symbols that have a length.
TP_RULE inline int canonical_decode(const uint32_t* count, const uint16_t* symbol, uint32_t bits, int max_len, int* len_out)
{
	uint32_t code = 0, first = 0, index = 0;
	for (int len = 1; len <= max_len; len++) {
		code |= bits & 1u;
		bits >>= 1;
		const uint32_t c = TP_INFLATE_UNIFORM(count[len]);
		if (code < first + c) { *len_out = len; return (int)TP_INFLATE_UNIFORM(symbol[index + (code - first)]); }
		index += c;
		first = (first + c) << 1;
		code <<= 1;
	}
	*len_out = 0;
	return -1;
}
// the same for one entry of a fast table, on a lane of its own (nothing here is wave-uniform)
TP_RULE inline uint16_t fast_entry(const uint32_t* count, const uint16_t* symbol, uint32_t bits, int fast_bits)
{
	uint32_t code = 0, first = 0, index = 0;
	for (int len = 1; len <= fast_bits; len++) {
		code |= bits & 1u;
		bits >>= 1;
		const uint32_t c = count[len];
		if (code < first + c) return (uint16_t)((uint32_t)symbol[index + (code - first)] << 4 | (uint32_t)len);
		index += c;
		first = (first + c) << 1;
		code <<= 1;
	}
	return 0;
}
// where symbol s of length l stands among the symbols sorted by (length, symbol)
TP_RULE inline uint32_t sorted_position(const uint8_t* len, const uint32_t* count, int s)
{
	const int l = len[s];
	uint32_t at = 0;
	for (int b = 1; b < l; b++) at += count[b];
	for (int t = 0; t < s; t++) at += len[t] == l ? 1u : 0u;
	return at;
}
// zlib's verdict on the counts of a code: over-subscribed, or incomplete where that is not allowed.  count[0] is not read.
TP_RULE inline Status judge_counts(const uint32_t* count, int max_bits, Kind kind)
{
	int32_t left = 1;
	int longest = 0;
	for (int l = 1; l <= max_bits; l++) {
		const uint32_t c = TP_INFLATE_UNIFORM(count[l]);
		left = left * 2 - (int32_t)c;                          // (at most 2^15 before a count of at most 320 is taken off)
		if (left < 0) return kBadCodeLengths;
		if (c) longest = l;
	}
	if (longest == 0) return kind == kCodes ? kBadCodeLengths : kOk;
	if (left > 0 && (kind == kCodes || longest != 1)) return kBadCodeLengths;
	return kOk;
}
// The decoding tables of the n code lengths len[0 .. n): all lanes.  fast may be null.
TP_RULE inline Status build_code(const uint8_t* len, int n, uint32_t* count, uint16_t* symbol, uint16_t* fast, int fast_bits, int max_bits, Kind kind)
{
	TP_INFLATE_LANES(lane) {
		for (int l = lane; l < 16; l += kLanes) count[l] = 0;
	}
	TP_INFLATE_LANES(lane) {
		for (int s = lane; s < n; s += kLanes) TP_DEFLATE_ADD(count[len[s] & 15], 1u);
	}
	TP_INFLATE_LANES(lane) {
		for (int s = lane; s < n; s += kLanes)
			if (len[s]) symbol[sorted_position(len, count, s)] = (uint16_t)s;
	}
	const Status verdict = judge_counts(count, max_bits, kind);
	if (verdict != kOk) return verdict;
	if (fast) {
		TP_INFLATE_LANES(lane) {
			for (uint32_t i = (uint32_t)lane; i < (1u << fast_bits); i += kLanes) fast[i] = fast_entry(count, symbol, i, fast_bits);
		}
	}
	return kOk;
}

// ---- bit reader ---------------------------------------------------------------------------------------------------------------------
// word w of the stream moved up by `shift` bytes: an aligned load where the word lies inside [src, src + n), single bytes (zero
// outside) at the two ends.  Nothing at or beyond src + n is read.
TP_RULE inline uint32_t stream_word(const unsigned char* src, uint64_t n, uint32_t shift, uint64_t w)
{
	const int64_t p0 = (int64_t)(4 * w) - (int64_t)shift;
	if (p0 >= (int64_t)n) return 0;
	if (p0 >= 0 && p0 + 4 <= (int64_t)n) return *reinterpret_cast<const uint32_t*>(src + p0);
	uint32_t v = 0;
	for (int k = 0; k < 4; k++)
		if (p0 + k >= 0 && p0 + k < (int64_t)n) v |= (uint32_t)src[p0 + k] << (8 * k);
	return v;
}
// the stage from word w0 on: all lanes
TP_RULE inline void refill(Lds& lds, State& st, uint64_t w0)
{
	st.w0 = w0;
	TP_INFLATE_LANES(lane) {
		for (uint32_t i = (uint32_t)lane; i < kStageWords; i += kLanes) lds.stage[i] = stream_word(st.src, st.n, st.shift, w0 + i);
	}
}
// 32 bits of the stream from bit st.pos on, least significant first; bits behind the stream's end are zero
TP_RULE inline uint32_t peek(Lds& lds, State& st)
{
	if (!st.hold_set || st.pos < st.hold_pos || st.pos + 32 > st.hold_pos + 64) {
		const uint64_t vb = (st.pos >> 3) + st.shift, wv = vb >> 2;
		if (wv < st.w0 || wv + 3 > st.w0 + kStageWords) refill(lds, st, wv);
		const uint32_t l = (uint32_t)(wv - st.w0);                 // l + 2 < kStageWords
		const uint64_t s0 = TP_INFLATE_UNIFORM(lds.stage[l]), s1 = TP_INFLATE_UNIFORM(lds.stage[l + 1]), s2 = TP_INFLATE_UNIFORM(lds.stage[l + 2]);
		const uint32_t sh = 8 * (uint32_t)(vb & 3);
		st.hold = (s0 | s1 << 32) >> sh | (sh ? s2 << (64 - sh) : (uint64_t)0);
		st.hold_pos = (st.pos >> 3) << 3;
		st.hold_set = true;
	}
	return (uint32_t)(st.hold >> (uint32_t)(st.pos - st.hold_pos));
}
// whether the next nbits bits lie inside the stream
TP_RULE inline bool has_bits(const State& st, uint32_t nbits) { return st.pos + nbits <= 8 * st.n; }

// ---- window -------------------------------------------------------------------------------------------------------------------------
TP_RULE inline unsigned char* window_bytes(Lds& lds) { return reinterpret_cast<unsigned char*>(lds.window); }
// where byte p of the output stands in the ring
TP_RULE inline uint32_t window_index(const State& st, uint64_t p) { return (uint32_t)((p + st.oshift) & (kWindow - 1)); }
// element k of a match of distance dist at output position out: its source and its target in the ring
TP_RULE inline uint32_t match_source(const State& st, uint32_t dist, uint32_t k) { return window_index(st, st.out - dist + k % dist); }
TP_RULE inline uint32_t match_target(const State& st, uint32_t k) { return window_index(st, st.out + k); }

// One linear piece [st.flushed, st.flushed + seg) of the ring to memory and into the CRC: all lanes.  Bytes up to the first aligned
// word and behind the last one go as bytes, what lies between as words; nothing outside dst[st.flushed, st.flushed + seg) is written.
TP_RULE inline void flush_piece(Lds& lds, State& st, uint32_t seg)
{
	const uint32_t wi = window_index(st, st.flushed);              // wi + seg <= kWindow
	const uint64_t vb = st.flushed + st.oshift, ve = vb + seg;     // the piece in addresses relative to dst - oshift, a multiple of 4
	uint64_t a = (vb + 3) & ~(uint64_t)3, b = ve & ~(uint64_t)3;
	if (a > ve) a = ve;
	if (b < a) b = a;
	TP_INFLATE_ONE_LANE lds.crc_acc = 0;
	TP_INFLATE_LANES(lane) {
		const uint32_t term = tp_deflate_rules::crc_slice_term(lds.crc_table, window_bytes(lds) + wi, seg, lane);
		if (term) TP_INFLATE_XOR(lds.crc_acc, term);
		for (uint64_t v = vb + (uint32_t)lane; v < a; v += kLanes) st.dst[v - st.oshift] = window_bytes(lds)[v & (kWindow - 1)];
		for (uint64_t v = a + 4 * (uint64_t)lane; v < b; v += 4 * kLanes) *reinterpret_cast<uint32_t*>(st.dst + (v - st.oshift)) = lds.window[(v & (kWindow - 1)) >> 2];
		for (uint64_t v = b + (uint32_t)lane; v < ve; v += kLanes) st.dst[v - st.oshift] = window_bytes(lds)[v & (kWindow - 1)];
	}
	st.crc = tp_deflate_rules::crc_combine(st.crc, TP_INFLATE_UNIFORM(lds.crc_acc), seg);
	st.flushed += seg;
}
// the finished bytes to memory: up to the last aligned word, or all of them at the end
TP_RULE inline void flush(Lds& lds, State& st, bool all)
{
	uint64_t target = st.out;
	if (!all) {
		const uint64_t t = (st.out + st.oshift) & ~(uint64_t)3;
		target = t > st.oshift ? t - st.oshift : 0;
	}
	while (st.flushed < target) {
		const uint32_t wi = window_index(st, st.flushed);
		const uint64_t left = target - st.flushed;
		flush_piece(lds, st, left < kWindow - wi ? (uint32_t)left : kWindow - wi);
	}
}
// room in the ring for nbytes (at most kWindow - 3) more bytes: unflushed bytes are never overwritten
TP_RULE inline void room(Lds& lds, State& st, uint32_t nbytes)
{
	if (st.out + nbytes > st.flushed + kWindow) flush(lds, st, false);
}

// ---- blocks -------------------------------------------------------------------------------------------------------------------------
// a stored block behind its three header bits
TP_RULE inline Status stored_block(Lds& lds, State& st)
{
	st.pos = (st.pos + 7) & ~(uint64_t)7;
	if (!has_bits(st, 32)) return kInputEnds;
	const uint32_t head = peek(lds, st);
	st.pos += 32;
	uint32_t left = head & 0xFFFFu;
	if ((left ^ 0xFFFFu) != head >> 16) return kStoredLength;
	uint64_t at = st.pos >> 3;
	if (at + left > st.n) return kInputEnds;
	if (st.out + left > st.capacity) return kOutputFull;
	while (left) {
		const uint32_t piece = left < kPiece ? left : kPiece;
		room(lds, st, piece);
		TP_INFLATE_LANES(lane) {
			for (uint32_t k = (uint32_t)lane; k < piece; k += kLanes) window_bytes(lds)[window_index(st, st.out + k)] = st.src[at + k];
		}
		st.out += piece;
		at += piece;
		left -= piece;
	}
	st.pos = 8 * at;
	return kOk;
}

// the code lengths of a fixed block
TP_RULE inline void fixed_lengths(Lds& lds)
{
	TP_INFLATE_LANES(lane) {
		for (int s = lane; s < kMaxLL; s += kLanes) lds.len[s] = (uint8_t)tp_deflate_rules::fixed_length_ll(s);
		for (int s = lane; s < kMaxD; s += kLanes) lds.len[kMaxLL + s] = (uint8_t)tp_deflate_rules::kFixedLengthD;
	}
}

// the header of a dynamic block: the code lengths into lds.len, hlit of the literal/length code, then hdist of the distance code
TP_RULE inline Status dynamic_header(Lds& lds, State& st, int* hlit_out, int* hdist_out)
{
	if (!has_bits(st, 14)) return kInputEnds;
	uint32_t bits = peek(lds, st);
	st.pos += 14;
	const int hlit = (int)(bits & 31u) + 257, hdist = (int)((bits >> 5) & 31u) + 1, hclen = (int)((bits >> 10) & 15u) + 4;
	if (hlit > 286 || hdist > 30) return kTooManySymbols;
	TP_INFLATE_LANES(lane) {
		for (int i = lane; i < 20; i += kLanes) lds.len_cl[i] = 0;
	}
	for (int i = 0; i < hclen; i++) {
		if (!has_bits(st, 3)) return kInputEnds;
		bits = peek(lds, st);
		st.pos += 3;
		TP_INFLATE_ONE_LANE lds.len_cl[tp_deflate_rules::cl_order(i)] = (uint8_t)(bits & 7u);
	}
	Status status = build_code(lds.len_cl, kNumCL, lds.count_cl, lds.sym_cl, nullptr, 0, kMaxBitsCL, kCodes);
	if (status != kOk) return status;
	const int total = hlit + hdist;
	int have = 0;
	uint32_t prev = 0, eob = 0;
	while (have < total) {
		int l = 0;
		bits = peek(lds, st);
		const int sym = canonical_decode(lds.count_cl, lds.sym_cl, bits, kMaxBitsCL, &l);
		if (sym < 0) return kBadSymbol;                            // (a complete code: not reached)
		if (!has_bits(st, (uint32_t)l)) return kInputEnds;
		st.pos += (uint32_t)l;
		if (sym < 16) {
			TP_INFLATE_ONE_LANE lds.len[have] = (uint8_t)sym;
			if (have == kEob) eob = (uint32_t)sym;
			prev = (uint32_t)sym;
			have++;
			continue;
		}
		if (sym == 16 && have == 0) return kBadCodeLengths;
		const uint32_t eb = (uint32_t)tp_deflate_rules::cl_extra_bits(sym);
		if (!has_bits(st, eb)) return kInputEnds;
		bits = peek(lds, st);
		st.pos += eb;
		const int rep = (sym == 18 ? 11 : 3) + (int)(bits & ((1u << eb) - 1u));
		const uint32_t v = sym == 16 ? prev : 0u;
		if (have + rep > total) return kBadCodeLengths;
		TP_INFLATE_LANES(lane) {
			for (int k = lane; k < rep; k += kLanes) lds.len[have + k] = (uint8_t)v;
		}
		if (have <= kEob && kEob < have + rep) eob = v;
		have += rep;
		prev = v;
	}
	if (eob == 0) return kNoEndOfBlock;
	*hlit_out = hlit;
	*hdist_out = hdist;
	return kOk;
}

// one symbol of a code with a fast table; returns the symbol or -1, and its length
TP_RULE inline int decode_symbol(const uint16_t* fast, int fast_bits, const uint32_t* count, const uint16_t* symbol, uint32_t bits, int* len_out)
{
	const uint32_t e = TP_INFLATE_UNIFORM(fast[bits & ((1u << fast_bits) - 1u)]);
	if (e & 15u) { *len_out = (int)(e & 15u); return (int)(e >> 4); }
	return canonical_decode(count, symbol, bits, kMaxBits, len_out);
}

// the symbols of a fixed or dynamic block, up to its end-of-block code, under the tables of lds
TP_RULE inline Status coded_block(Lds& lds, State& st)
{
	for (;;) {
		int l = 0;
		uint32_t bits = peek(lds, st);
		const int sym = decode_symbol(lds.fast_ll, kFastBitsLL, lds.count_ll, lds.sym_ll, bits, &l);
		if (sym < 0) return kBadSymbol;
		if (!has_bits(st, (uint32_t)l)) return kInputEnds;
		st.pos += (uint32_t)l;
		if (sym < kEob) {
			if (st.out + 1 > st.capacity) return kOutputFull;
			room(lds, st, 1);
			TP_INFLATE_ONE_LANE window_bytes(lds)[window_index(st, st.out)] = (unsigned char)sym;
			st.out++;
			continue;
		}
		if (sym == kEob) return kOk;
		if (sym >= 286) return kBadSymbol;
		uint32_t eb = (uint32_t)tp_deflate_rules::length_extra_bits(sym);
		if (!has_bits(st, eb)) return kInputEnds;
		bits = peek(lds, st);
		st.pos += eb;
		const uint32_t length = length_base(sym) + (bits & ((1u << eb) - 1u));
		bits = peek(lds, st);
		const int dsym = decode_symbol(lds.fast_d, kFastBitsD, lds.count_d, lds.sym_d, bits, &l);
		if (dsym < 0) return kBadSymbol;
		if (!has_bits(st, (uint32_t)l)) return kInputEnds;
		st.pos += (uint32_t)l;
		if (dsym >= 30) return kBadSymbol;
		eb = (uint32_t)tp_deflate_rules::distance_extra_bits(dsym);
		if (!has_bits(st, eb)) return kInputEnds;
		bits = peek(lds, st);
		st.pos += eb;
		const uint32_t dist = distance_base(dsym) + (bits & ((1u << eb) - 1u));
		if (dist > st.out) return kDistanceTooFar;
		if (st.out + length > st.capacity) return kOutputFull;
		room(lds, st, length);
		// rows of 64 elements, a row read before it is written: with dist > kWindow - 258 a later element's target is an earlier element's source
		for (uint32_t k0 = 0; k0 < length; k0 += kLanes) {
			unsigned char v[TP_INFLATE_SLOTS];
			TP_INFLATE_LANES(lane) {
				if (k0 + (uint32_t)lane < length) v[TP_INFLATE_SLOT(lane)] = window_bytes(lds)[match_source(st, dist, k0 + (uint32_t)lane)];
			}
			TP_INFLATE_LANES(lane) {
				if (k0 + (uint32_t)lane < length) window_bytes(lds)[match_target(st, k0 + (uint32_t)lane)] = v[TP_INFLATE_SLOT(lane)];
			}
		}
		st.out += length;
	}
}

// ---- a stream -----------------------------------------------------------------------------------------------------------------------
// The raw deflate stream [src, src + n) into the slot [dst, dst + capacity): blocks up to the one with BFINAL, or up to the first
// rule broken.  What was produced before that is in the slot, counted and summed; in_bytes is the bytes up to the final block's last
// bit (the whole input when the status is not OK).
TP_RULE inline Result inflate_stream(Lds& lds, const unsigned char* src, uint64_t n, uint32_t src_shift, unsigned char* dst, uint64_t capacity, uint32_t dst_shift)
{
	State st;
	st.src = src; st.n = n; st.shift = src_shift;
	st.pos = 0; st.hold = 0; st.hold_pos = 0; st.hold_set = false;
	st.dst = dst; st.capacity = capacity; st.oshift = dst_shift;
	st.out = 0; st.flushed = 0; st.crc = 0;
	TP_INFLATE_LANES(lane) {
		for (int i = lane; i < 256; i += kLanes) lds.crc_table[i] = tp_deflate_rules::crc_table_entry((uint32_t)i);
	}
	refill(lds, st, 0);
	Status status = kOk;
	bool last = false;
	while (status == kOk && !last) {
		if (!has_bits(st, 3)) { status = kInputEnds; break; }
		const uint32_t bits = peek(lds, st);
		st.pos += 3;
		last = (bits & 1u) != 0;
		const uint32_t type = (bits >> 1) & 3u;
		if (type == 0) {
			status = stored_block(lds, st);
		} else if (type == 3) {
			status = kBadBlockType;
		} else {
			int hlit = kMaxLL, hdist = kMaxD;
			if (type == 1) fixed_lengths(lds);
			else status = dynamic_header(lds, st, &hlit, &hdist);
			if (status == kOk) status = build_code(lds.len, hlit, lds.count_ll, lds.sym_ll, lds.fast_ll, kFastBitsLL, kMaxBits, kLens);
			if (status == kOk) status = build_code(lds.len + hlit, hdist, lds.count_d, lds.sym_d, lds.fast_d, kFastBitsD, kMaxBits, kDists);
			if (status == kOk) status = coded_block(lds, st);
		}
	}
	flush(lds, st, true);
	Result r;
	r.status = (int32_t)status;
	r.out_bytes = st.out;
	r.in_bytes = status == kOk ? (st.pos + 7) >> 3 : n;
	r.crc = st.crc;
	return r;
}

} // namespace tp_inflate_rules
