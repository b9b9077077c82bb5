// deflate_rules.h -- what the batched DEFLATE encoder decides (deflate.hip; RFC 1951), each rule stated once over plain values: how a
// stream is cut into chunks, what a chunk's output is, the length / distance code tables and the LSB-first bit writer, the matcher
// (hash, candidate, length count, table update, greedy parse), the construction of the length-limited prefix codes and of the block
// header, the choice between the dynamic, fixed and stored forms by exact size, CRC-32 with its combine operator, and the refusals
// of tp_deflate.  No device code, no HIP runtime: the kernel calls these from its wavefront's plumbing (ballots, prefix sums,
// barriers), tests/hostsim/deflate_rules_host.cpp composes them serially -- every chunk, every lane -- into the bytes the kernel
// writes under AddressSanitizer and UBSan, and tests/test_deflate_rules_host.py inflates those with zlib.
//
// A chunk is TP_DEFLATE_CHUNK input bytes (the last one of a stream shorter) with a window of its own: no match reaches before the
// chunk, the largest distance is chunk - 1.  Its output is a byte-aligned run of complete blocks without BFINAL -- one dynamic or
// fixed block followed by an empty stored block (000, pad, 00 00 FF FF: what Z_SYNC_FLUSH and pigz write), or one stored block --,
// so the chunks of a stream are concatenated as they are, and `03 00` behind the last one ends the stream.
//
// One wavefront owns a chunk; its state is the struct Lds below (36.5 KiB: four chunks per CU).  Everything that several lanes write
// goes through TP_DEFLATE_MAX / _ADD / _OR: integer maximum, sum and bitwise or, whose results do not depend on the order of the
// lanes -- LDS atomics in the kernel, plain statements in the serial composition.  The output is a function of the input bytes alone.
#pragma once
#include <cstdint>
#include "fits_rules.h"

#define TP_DEFLATE_CHUNK 16384

#if defined(__HIP_DEVICE_COMPILE__)
#define TP_DEFLATE_MAX(ref, v) atomicMax(&(ref), (v))
#define TP_DEFLATE_ADD(ref, v) atomicAdd(&(ref), (v))
#define TP_DEFLATE_OR(ref, v) atomicOr(&(ref), (v))
#else
#define TP_DEFLATE_MAX(ref, v) do { if ((v) > (ref)) (ref) = (v); } while (0)
#define TP_DEFLATE_ADD(ref, v) do { (ref) += (v); } while (0)
#define TP_DEFLATE_OR(ref, v) do { (ref) |= (v); } while (0)
#endif

namespace tp_deflate_rules {

constexpr int kChunk = TP_DEFLATE_CHUNK;
constexpr int kLanes = 64;                 // a wavefront
constexpr int kMinMatch = 4;               // the hash covers four bytes; a three-byte match at a noise table's distances costs more than its literals
constexpr int kMaxMatch = 258;
constexpr int kHashBits = 12;
constexpr int kHashSize = 1 << kHashBits;
constexpr int kNumLL = 286, kNumD = 30, kNumCL = 19;
constexpr int kEob = 256;
constexpr int kMaxBitsLL = 15, kMaxBitsCL = 7;
constexpr int kStoredHead = 5;             // 000 + pad, LEN, NLEN
constexpr int kChunkGrowth = kStoredHead;  // a chunk's output never exceeds its input by more: the stored form needs no closer
constexpr int kSlotBytes = 16400;          // a chunk's pitched output in the work buffer: kChunk + kChunkGrowth, whole words, 16-byte multiple
constexpr int kStageWords = 256;           // LDS words the bit writer fills between two flushes (header: at most 141; 64 tokens: at most 97)
constexpr int kTokenBytes = 4 * kChunk;    // a chunk's tokens in the work buffer
constexpr uint64_t kMaxTotal = (uint64_t)1 << 34;
constexpr uint32_t kCrcPoly = 0xEDB88320u; // the gzip polynomial, reflected

enum Form { kFormStored = 0, kFormFixed = 1, kFormDynamic = 2 };

// one chunk of a call: where its input begins in d_in, and its length
struct ChunkDesc {
	uint64_t offset;
	uint32_t nbytes;
	uint32_t pad;
};

// the state of a chunk: LDS in the kernel
struct Lds {
	uint32_t in_words[kChunk / 4 + 2];     // the input, moved up by (address & 3) bytes so that aligned words of memory are aligned words here
	union {
		uint32_t hash[kHashSize];          // matcher: position + 1 of the latest earlier occurrence, 0 = none
		struct {                           // code builder, after the parse
			uint32_t a[288];
			uint16_t sorted[288];
			uint16_t cl_seq[320];          // the run-length coded code lengths: symbol | extra << 8
		} b;
	} u;
	uint32_t freq_ll[288], freq_d[32], freq_cl[20];
	uint32_t count[16], next_code[16];
	uint16_t code_ll[288], code_d[32], code_cl[20];
	uint8_t len_ll[288], len_d[32], len_cl[20];
	uint32_t stage[kStageWords];
	uint32_t crc_table[256];
	uint32_t n_seq, hlit, hdist, hclen, form, coded_bytes;
};

// ---- chunking and bounds ----------------------------------------------------------------------------------------------------------
TP_RULE inline uint64_t n_chunks_of(uint64_t nbytes) { return (nbytes + kChunk - 1) / kChunk; }
TP_RULE inline uint64_t bound_of(uint64_t nbytes) { return nbytes + (uint64_t)kChunkGrowth * n_chunks_of(nbytes); }

// the work buffer of a call with n chunks: chunk table, chunk sizes, tokens, pitched outputs -- each part a multiple of 16 bytes
struct WorkLayout {
	uint64_t table, sizes, tokens, slots, total;
};
TP_RULE inline WorkLayout work_layout(uint64_t n_chunks)
{
	WorkLayout w;
	w.table = 0;
	w.sizes = w.table + n_chunks * sizeof(ChunkDesc);
	w.tokens = w.sizes + ((n_chunks * 4 + 15) / 16) * 16;
	w.slots = w.tokens + n_chunks * (uint64_t)kTokenBytes;
	w.total = w.slots + n_chunks * (uint64_t)kSlotBytes;
	return w;
}

// the message of the first rule a call of tp_deflate breaks, or null.  Addresses travel as integers; `offsets` is host memory.
// Alignments: d_in and d_out none (bytes), d_chunk_end 8, d_chunk_crc 4, d_work 16.
inline const char* check(uint64_t in_addr, const uint64_t* offsets, int64_t n_streams, uint64_t out_addr, uint64_t out_capacity, uint64_t end_addr,
	uint64_t crc_addr, uint64_t work_addr, uint64_t work_bytes, uint64_t* n_chunks_out)
{
	if (n_chunks_out) *n_chunks_out = 0;
	if (n_streams < 1) return "tp_deflate: n_streams must be at least 1";
	if (offsets == nullptr) return "tp_deflate: null pointer";
	for (int64_t s = 0; s < n_streams; s++)
		if (offsets[s + 1] < offsets[s]) return "tp_deflate: the stream offsets must not fall";
	if (offsets[n_streams] - offsets[0] >= kMaxTotal || offsets[n_streams] >= ((uint64_t)1 << 62)) return "tp_deflate: a call holds fewer than 2^34 bytes";
	uint64_t chunks = 0, bound = 0;
	for (int64_t s = 0; s < n_streams; s++) {
		chunks += n_chunks_of(offsets[s + 1] - offsets[s]);
		bound += bound_of(offsets[s + 1] - offsets[s]);
	}
	if (n_chunks_out) *n_chunks_out = chunks;
	if (chunks == 0) return nullptr;                       // nothing to do: no pointer is read
	if (in_addr == 0 || out_addr == 0 || end_addr == 0 || crc_addr == 0 || work_addr == 0) return "tp_deflate: null pointer";
	if (end_addr % 8 != 0) return "tp_deflate: d_chunk_end must be 8-byte aligned";
	if (crc_addr % 4 != 0) return "tp_deflate: d_chunk_crc must be 4-byte aligned";
	if (work_addr % 16 != 0) return "tp_deflate: d_work must be 16-byte aligned";
	if (out_capacity < bound) return "tp_deflate: out_capacity is below the sum of tp_deflate_bound over the streams";
	if (work_bytes < work_layout(chunks).total) return "tp_deflate: the work buffer is smaller than tp_deflate_work_bytes";
	return nullptr;
}

// the chunk table of a call, in call order; `table` holds n_chunks entries
inline void chunk_table(const uint64_t* offsets, int64_t n_streams, ChunkDesc* table)
{
	uint64_t c = 0;
	for (int64_t s = 0; s < n_streams; s++)
		for (uint64_t at = offsets[s]; at < offsets[s + 1]; at += kChunk) {
			const uint64_t left = offsets[s + 1] - at;
			table[c++] = ChunkDesc{at, (uint32_t)(left < (uint64_t)kChunk ? left : (uint64_t)kChunk), 0u};
		}
}

// ---- state ----------------------------------------------------------------------------------------------------------------------
// a chunk's state before its first byte, lane `lane` of `lanes`: empty hash table, counts (the end-of-block symbol occurs once),
// an empty stage, and the CRC table
TP_RULE inline uint32_t crc_table_entry(uint32_t i);
TP_RULE inline void reset(Lds& lds, int lane, int lanes)
{
	for (int i = lane; i < kHashSize; i += lanes) lds.u.hash[i] = 0;
	for (int i = lane; i < 288; i += lanes) lds.freq_ll[i] = i == kEob ? 1u : 0u;
	for (int i = lane; i < 32; i += lanes) lds.freq_d[i] = 0;
	for (int i = lane; i < kStageWords; i += lanes) lds.stage[i] = 0;
	for (int i = lane; i < 256; i += lanes) lds.crc_table[i] = crc_table_entry((uint32_t)i);
}

// ---- load -----------------------------------------------------------------------------------------------------------------------
// Word w of Lds::in_words for a chunk of n bytes at `src`, shift = address of src & 3: an aligned load where the word lies inside
// the chunk, single bytes (zero outside) at its two ends.  Nothing outside [src, src + n) is read.
TP_RULE inline uint32_t load_word(const unsigned char* src, uint32_t n, uint32_t shift, uint32_t w)
{
	const int64_t p0 = (int64_t)4 * w - shift;             // chunk byte that lands in the word's low byte
	if (p0 >= 0 && p0 + 4 <= (int64_t)n) return *reinterpret_cast<const uint32_t*>(src + p0);
	uint32_t v = 0;
	for (int k = 0; k < 4; k++)
		if (p0 + k >= 0 && p0 + k < (int64_t)n) v |= (uint32_t)src[p0 + k] << (8 * k);
	return v;
}
TP_RULE inline uint32_t load_words(uint32_t n, uint32_t shift) { return (n + shift + 3) / 4; }
TP_RULE inline const unsigned char* input_of(const Lds& lds, uint32_t shift) { return reinterpret_cast<const unsigned char*>(lds.in_words) + shift; }

// ---- code tables ------------------------------------------------------------------------------------------------------------------
TP_RULE inline int high_bit(uint32_t v) { return 31 - __builtin_clz(v); }          // v > 0
// length 3 .. 258 -> symbol 257 .. 285 and its extra bits (RFC 1951, 3.2.5): eight symbols without extra bits, then four per bit count
TP_RULE inline int length_symbol(int len, int* extra_bits, int* extra)
{
	const int l = len - 3;
	if (len == kMaxMatch) { *extra_bits = 0; *extra = 0; return 285; }
	if (l < 8) { *extra_bits = 0; *extra = 0; return 257 + l; }
	const int e = high_bit((uint32_t)l) - 2;
	*extra_bits = e;
	*extra = l & ((1 << e) - 1);
	return 257 + 4 * e + 4 + ((l >> e) & 3);
}
// distance 1 .. 32768 -> symbol 0 .. 29 and its extra bits: four symbols without, then two per bit count
TP_RULE inline int distance_symbol(int dist, int* extra_bits, int* extra)
{
	const int d = dist - 1;
	if (d < 4) { *extra_bits = 0; *extra = 0; return d; }
	const int nb = high_bit((uint32_t)d);
	*extra_bits = nb - 1;
	*extra = d & ((1 << (nb - 1)) - 1);
	return 2 * nb + ((d >> (nb - 1)) & 1);
}
TP_RULE inline int length_extra_bits(int sym) { return (sym < 265 || sym >= 285) ? 0 : (sym - 261) / 4; }
TP_RULE inline int distance_extra_bits(int sym) { return sym < 4 ? 0 : sym / 2 - 1; }
TP_RULE inline int fixed_length_ll(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
constexpr int kFixedLengthD = 5;
// the order in which the lengths of the code-length alphabet are sent
TP_RULE inline int cl_order(int i)
{
	const unsigned char order[kNumCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
	return order[i];
}
TP_RULE inline int cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }
// a Huffman code is sent most significant bit first: kept bit-reversed for the LSB-first writer
TP_RULE inline uint32_t reverse_bits(uint32_t code, int len)
{
	uint32_t r = 0;
	for (int i = 0; i < len; i++) r |= ((code >> i) & 1u) << (len - 1 - i);
	return r;
}

// ---- bit writer -------------------------------------------------------------------------------------------------------------------
// nbits (<= 48) of `bits`, least significant first, at bit `at` of the stage: up to three words, or-ed in (several lanes at once)
TP_RULE inline void or_bits(uint32_t* stage, uint32_t at, uint64_t bits, int nbits)
{
	if (nbits == 0) return;
	const uint32_t w = at >> 5, o = at & 31;
	const uint64_t lo = bits << o;
	const uint32_t hi = o ? (uint32_t)(bits >> (64 - o)) : 0u;
	if ((uint32_t)lo) TP_DEFLATE_OR(stage[w], (uint32_t)lo);
	if ((uint32_t)(lo >> 32)) TP_DEFLATE_OR(stage[w + 1], (uint32_t)(lo >> 32));
	if (hi) TP_DEFLATE_OR(stage[w + 2], hi);
}
// the serial writer of one lane
TP_RULE inline void put_bits(uint32_t* stage, uint32_t* at, uint32_t bits, int nbits)
{
	or_bits(stage, *at, bits, nbits);
	*at += (uint32_t)nbits;
}

// ---- matcher ----------------------------------------------------------------------------------------------------------------------
TP_RULE inline uint32_t read4(const unsigned char* in, uint32_t p) { return (uint32_t)in[p] | (uint32_t)in[p + 1] << 8 | (uint32_t)in[p + 2] << 16 | (uint32_t)in[p + 3] << 24; }
TP_RULE inline uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }
// bytes that agree at a and b (a < b), at most `most`
TP_RULE inline uint32_t match_length(const unsigned char* in, uint32_t a, uint32_t b, uint32_t most)
{
	uint32_t k = 0;
	while (k < most && in[a + k] == in[b + k]) k++;
	return k;
}
// The match at position p of a chunk of n bytes, as length << 16 | distance, or 0: the longer of the table's candidate -- the latest
// position before `base`, the first position of p's group of 64, whose four bytes hash as p's do -- and of distance 1, the shorter
// distance at equal length.  Positions of p's own group are not in the table yet: a group reads the table, then updates it.
TP_RULE inline uint32_t find_match(const unsigned char* in, const uint32_t* hash, uint32_t p, uint32_t n)
{
	if (p + kMinMatch > n) return 0;
	const uint32_t most = n - p < (uint32_t)kMaxMatch ? n - p : (uint32_t)kMaxMatch;
	uint32_t best = 0, dist = 0;
	const uint32_t entry = hash[hash4(read4(in, p))];
	if (entry != 0) {
		const uint32_t len = match_length(in, entry - 1, p, most);
		if (len >= (uint32_t)kMinMatch) { best = len; dist = p - (entry - 1); }
	}
	if (p >= 1 && dist != 1) {
		const uint32_t len = match_length(in, p - 1, p, most);
		if (len >= (uint32_t)kMinMatch && len >= best) { best = len; dist = 1; }
	}
	return best ? best << 16 | dist : 0;
}
// the table update of position p: the highest position wins, whichever lane comes first
TP_RULE inline void hash_insert(const unsigned char* in, uint32_t* hash, uint32_t p, uint32_t n)
{
	if (p + kMinMatch > n) return;
	TP_DEFLATE_MAX(hash[hash4(read4(in, p))], p + 1);
}
// greedy parse of a group: the first lane at or behind `from` that holds a match, 64 when there is none (match_mask: bit l = lane l)
TP_RULE inline int next_match_lane(uint64_t match_mask, int from)
{
	const uint64_t m = from >= 64 ? 0 : (match_mask >> from) << from;
	return m ? __builtin_ctzll(m) : 64;
}

// ---- tokens -----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kTokenMatch = 0x80000000u;
TP_RULE inline uint32_t literal_token(unsigned char b) { return b; }
TP_RULE inline uint32_t match_token(uint32_t match) { return kTokenMatch | match; }
// symbol counts of a token
TP_RULE inline void count_token(Lds& lds, uint32_t token)
{
	if (token & kTokenMatch) {
		int eb, e;
		TP_DEFLATE_ADD(lds.freq_ll[length_symbol((int)((token >> 16) & 0x1FF), &eb, &e)], 1u);
		TP_DEFLATE_ADD(lds.freq_d[distance_symbol((int)(token & 0xFFFF), &eb, &e)], 1u);
	} else {
		TP_DEFLATE_ADD(lds.freq_ll[token], 1u);
	}
}
// the bits of a token under the codes of lds (at most 48), least significant first
TP_RULE inline uint64_t token_bits(const Lds& lds, uint32_t token, int* nbits)
{
	if (!(token & kTokenMatch)) { *nbits = lds.len_ll[token]; return lds.code_ll[token]; }
	int leb, le, deb, de;
	const int ls = length_symbol((int)((token >> 16) & 0x1FF), &leb, &le);
	const int ds = distance_symbol((int)(token & 0xFFFF), &deb, &de);
	uint64_t bits = lds.code_ll[ls];
	int at = lds.len_ll[ls];
	bits |= (uint64_t)le << at; at += leb;
	bits |= (uint64_t)lds.code_d[ds] << at; at += lds.len_d[ds];
	bits |= (uint64_t)de << at; at += deb;
	*nbits = at;
	return bits;
}

// ---- code construction ------------------------------------------------------------------------------------------------------------
// Where used symbol s stands when the used symbols are sorted by (count, symbol) rising: one lane per symbol in the kernel
TP_RULE inline int rank_of(const uint32_t* freq, int n, int s)
{
	int r = 0;
	const uint32_t f = freq[s];
	for (int t = 0; t < n; t++) r += (freq[t] != 0 && (freq[t] < f || (freq[t] == f && t < s))) ? 1 : 0;
	return r;
}
TP_RULE inline void sort_symbols(const uint32_t* freq, int n, uint16_t* sorted, int lane, int lanes)
{
	for (int s = lane; s < n; s += lanes)
		if (freq[s] != 0) sorted[rank_of(freq, n, s)] = (uint16_t)s;
}
// Code lengths of the symbols sorted[0 .. used) (counts rising), at most max_bits, into len[0 .. n): one lane.  Huffman's code by the
// in-place method of Moffat and Katajainen on a[]; then depths above max_bits are cut to it and the Kraft sum is brought back to 1
// by lengthening the deepest shorter codes one at a time, and the lengths are dealt out again, the longest to the rarest.  One used
// symbol gets one bit and so does a second, unused one (symbol 0 or 1): inflate implementations refuse a code-length or
// literal/length code that is not complete.  No used symbol: all lengths 0.
TP_RULE inline void build_lengths(const uint32_t* freq, int n, int max_bits, uint8_t* len, const uint16_t* sorted, uint32_t* a, uint32_t* count)
{
	int used = 0;
	for (int s = 0; s < n; s++) { len[s] = 0; used += freq[s] != 0 ? 1 : 0; }
	if (used == 0) return;
	if (used == 1) {
		const int s = sorted[0];
		len[s] = 1;
		len[s == 0 ? 1 : 0] = 1;
		return;
	}
	for (int i = 0; i < used; i++) a[i] = freq[sorted[i]];
	// phase 1: parents
	a[0] += a[1];
	int root = 0, leaf = 2;
	for (int next = 1; next < used - 1; next++) {
		if (leaf >= used || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; } else a[next] = a[leaf++];
		if (leaf >= used || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; } else a[next] += a[leaf++];
	}
	// phase 2: depths of the internal nodes
	a[used - 2] = 0;
	for (int next = used - 3; next >= 0; next--) a[next] = a[a[next]] + 1;
	// phase 3: depths of the leaves
	int avbl = 1, inner = 0, depth = 0;
	root = used - 2;
	int next = used - 1;
	while (avbl > 0) {
		while (root >= 0 && (int)a[root] == depth) { inner++; root--; }
		while (avbl > inner) { a[next--] = (uint32_t)depth; avbl--; }
		avbl = 2 * inner;
		depth++;
		inner = 0;
	}
	// limit: a[i] is the depth of sorted[i], falling with i
	for (int b = 0; b <= max_bits; b++) count[b] = 0;
	for (int i = 0; i < used; i++) count[(int)a[i] < max_bits ? a[i] : (uint32_t)max_bits]++;
	uint32_t total = 0;
	for (int b = max_bits; b > 0; b--) total += count[b] << (max_bits - b);
	while (total != (1u << max_bits)) {
		count[max_bits]--;
		for (int b = max_bits - 1; b > 0; b--)
			if (count[b]) { count[b]--; count[b + 1] += 2; break; }
		total--;
	}
	int i = 0;
	for (int b = max_bits; b > 0; b--)
		for (uint32_t k = 0; k < count[b]; k++) len[sorted[i++]] = (uint8_t)b;
}
// canonical codes (RFC 1951, 3.2.2), bit-reversed: one lane
TP_RULE inline void assign_codes(const uint8_t* len, int n, int max_bits, uint16_t* code, uint32_t* count, uint32_t* next_code)
{
	for (int b = 0; b <= max_bits; b++) count[b] = 0;
	for (int s = 0; s < n; s++) count[len[s]]++;
	count[0] = 0;
	uint32_t c = 0;
	next_code[0] = 0;
	for (int b = 1; b <= max_bits; b++) { c = (c + count[b - 1]) << 1; next_code[b] = c; }
	for (int s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)reverse_bits(next_code[len[s]]++, len[s]) : (uint16_t)0;
}
// The code lengths of the two alphabets, hlit + hdist of them in one sequence, run-length coded with 16 (the previous length 3 .. 6
// more times), 17 (3 .. 10 zeros) and 18 (11 .. 138 zeros) into cl_seq, and the counts of the code-length symbols.  One lane.
TP_RULE inline uint8_t header_length(const Lds& lds, int i) { return i < (int)lds.hlit ? lds.len_ll[i] : lds.len_d[i - (int)lds.hlit]; }
TP_RULE inline void code_length_sequence(Lds& lds)
{
	int hlit = kNumLL, hdist = kNumD;
	while (hlit > 257 && lds.len_ll[hlit - 1] == 0) hlit--;
	while (hdist > 1 && lds.len_d[hdist - 1] == 0) hdist--;
	lds.hlit = (uint32_t)hlit;
	lds.hdist = (uint32_t)hdist;
	for (int s = 0; s < kNumCL; s++) lds.freq_cl[s] = 0;
	const int total = hlit + hdist;
	int n = 0, i = 0;
	while (i < total) {
		const int v = header_length(lds, i);
		int run = 1;
		while (i + run < total && header_length(lds, i + run) == v) run++;
		i += run;
		if (v == 0) {
			while (run >= 11) { const int r = run < 138 ? run : 138; lds.u.b.cl_seq[n++] = (uint16_t)(18 | (r - 11) << 8); lds.freq_cl[18]++; run -= r; }
			if (run >= 3) { lds.u.b.cl_seq[n++] = (uint16_t)(17 | (run - 3) << 8); lds.freq_cl[17]++; run = 0; }
		} else {
			lds.u.b.cl_seq[n++] = (uint16_t)v; lds.freq_cl[v]++; run--;
			while (run >= 3) { const int r = run < 6 ? run : 6; lds.u.b.cl_seq[n++] = (uint16_t)(16 | (r - 3) << 8); lds.freq_cl[16]++; run -= r; }
		}
		for (; run > 0; run--) { lds.u.b.cl_seq[n++] = (uint16_t)v; lds.freq_cl[v]++; }
	}
	lds.n_seq = (uint32_t)n;
}
// HCLEN: the code-length lengths sent, in cl_order, at least 4
TP_RULE inline void header_counts(Lds& lds)
{
	int hclen = kNumCL;
	while (hclen > 4 && lds.len_cl[cl_order(hclen - 1)] == 0) hclen--;
	lds.hclen = (uint32_t)hclen;
}
// exact bits of the block in its dynamic and its fixed form, header and end-of-block code included
TP_RULE inline uint64_t dynamic_bits(const Lds& lds)
{
	uint64_t bits = 3 + 5 + 5 + 4 + 3 * (uint64_t)lds.hclen;
	for (uint32_t k = 0; k < lds.n_seq; k++) { const int s = lds.u.b.cl_seq[k] & 0xFF; bits += (uint64_t)lds.len_cl[s] + (uint64_t)cl_extra_bits(s); }
	for (int s = 0; s < kNumLL; s++) bits += (uint64_t)lds.freq_ll[s] * (uint64_t)(lds.len_ll[s] + length_extra_bits(s));
	for (int s = 0; s < kNumD; s++) bits += (uint64_t)lds.freq_d[s] * (uint64_t)(lds.len_d[s] + distance_extra_bits(s));
	return bits;
}
TP_RULE inline uint64_t fixed_bits(const Lds& lds)
{
	uint64_t bits = 3;
	for (int s = 0; s < kNumLL; s++) bits += (uint64_t)lds.freq_ll[s] * (uint64_t)(fixed_length_ll(s) + length_extra_bits(s));
	for (int s = 0; s < kNumD; s++) bits += (uint64_t)lds.freq_d[s] * (uint64_t)(kFixedLengthD + distance_extra_bits(s));
	return bits;
}
// bytes of a chunk's output: a coded block of `bits` bits, then 000, the pad to a byte and 00 00 FF FF; or the stored form
TP_RULE inline uint64_t coded_bytes(uint64_t bits) { return (bits + 3 + 7) / 8 + 4; }
TP_RULE inline uint64_t stored_bytes(uint32_t n) { return (uint64_t)n + kStoredHead; }
// Everything between the parse and the emission, on one lane, with the symbols of the literal/length alphabet already sorted:
// the three codes, the header, and the form -- the smallest output; fixed before dynamic and stored before both at equal size.
// For the fixed form the code tables are overwritten with the fixed codes, so that the emission is the same.
TP_RULE inline void build_codes(Lds& lds, uint32_t n)
{
	build_lengths(lds.freq_ll, kNumLL, kMaxBitsLL, lds.len_ll, lds.u.b.sorted, lds.u.b.a, lds.count);
	sort_symbols(lds.freq_d, kNumD, lds.u.b.sorted, 0, 1);
	build_lengths(lds.freq_d, kNumD, kMaxBitsLL, lds.len_d, lds.u.b.sorted, lds.u.b.a, lds.count);
	code_length_sequence(lds);
	sort_symbols(lds.freq_cl, kNumCL, lds.u.b.sorted, 0, 1);
	build_lengths(lds.freq_cl, kNumCL, kMaxBitsCL, lds.len_cl, lds.u.b.sorted, lds.u.b.a, lds.count);
	header_counts(lds);
	const uint64_t dyn = coded_bytes(dynamic_bits(lds)), fix = coded_bytes(fixed_bits(lds)), sto = stored_bytes(n);
	if (sto <= dyn && sto <= fix) { lds.form = kFormStored; lds.coded_bytes = (uint32_t)sto; return; }
	if (fix <= dyn) {
		lds.form = kFormFixed;
		lds.coded_bytes = (uint32_t)fix;
		for (int s = 0; s < 288; s++) lds.len_ll[s] = (uint8_t)fixed_length_ll(s);
		for (int s = 0; s < 32; s++) lds.len_d[s] = (uint8_t)kFixedLengthD;
		assign_codes(lds.len_ll, 288, kMaxBitsLL, lds.code_ll, lds.count, lds.next_code);
		assign_codes(lds.len_d, 32, kMaxBitsLL, lds.code_d, lds.count, lds.next_code);
		return;
	}
	lds.form = kFormDynamic;
	lds.coded_bytes = (uint32_t)dyn;
	assign_codes(lds.len_ll, kNumLL, kMaxBitsLL, lds.code_ll, lds.count, lds.next_code);
	assign_codes(lds.len_d, kNumD, kMaxBitsLL, lds.code_d, lds.count, lds.next_code);
	assign_codes(lds.len_cl, kNumCL, kMaxBitsCL, lds.code_cl, lds.count, lds.next_code);
}
// the block header into the stage (one lane); returns the bits written
TP_RULE inline uint32_t put_header(Lds& lds)
{
	uint32_t at = 0;
	if (lds.form == kFormFixed) { put_bits(lds.stage, &at, 0u | 1u << 1, 3); return at; }       // BFINAL 0, BTYPE 01
	put_bits(lds.stage, &at, 0u | 2u << 1, 3);                                                   // BFINAL 0, BTYPE 10
	put_bits(lds.stage, &at, lds.hlit - 257, 5);
	put_bits(lds.stage, &at, lds.hdist - 1, 5);
	put_bits(lds.stage, &at, lds.hclen - 4, 4);
	for (uint32_t i = 0; i < lds.hclen; i++) put_bits(lds.stage, &at, lds.len_cl[cl_order((int)i)], 3);
	for (uint32_t k = 0; k < lds.n_seq; k++) {
		const int s = lds.u.b.cl_seq[k] & 0xFF;
		put_bits(lds.stage, &at, lds.code_cl[s], lds.len_cl[s]);
		put_bits(lds.stage, &at, (uint32_t)(lds.u.b.cl_seq[k] >> 8), cl_extra_bits(s));
	}
	return at;
}
// the end of a coded chunk at bit `at` of the stage (one lane): end-of-block, 000, the pad to a byte, 00 00 FF FF; returns the bits
TP_RULE inline uint32_t put_tail(Lds& lds, uint32_t at)
{
	put_bits(lds.stage, &at, lds.code_ll[kEob], lds.len_ll[kEob]);
	put_bits(lds.stage, &at, 0u, 3);
	at = (at + 7) & ~7u;
	put_bits(lds.stage, &at, 0xFFFF0000u, 32);
	return at;
}
// byte k of a chunk's stored form: 00, LEN, NLEN, the input
TP_RULE inline uint32_t stored_byte(const unsigned char* in, uint32_t n, uint32_t k)
{
	if (k >= n + kStoredHead) return 0;
	if (k >= (uint32_t)kStoredHead) return in[k - kStoredHead];
	return k == 0 ? 0u : k == 1 ? (n & 0xFF) : k == 2 ? (n >> 8) : k == 3 ? (~n & 0xFF) : ((~n >> 8) & 0xFF);
}
TP_RULE inline uint32_t stored_word(const unsigned char* in, uint32_t n, uint32_t w)
{
	return stored_byte(in, n, 4 * w) | stored_byte(in, n, 4 * w + 1) << 8 | stored_byte(in, n, 4 * w + 2) << 16 | stored_byte(in, n, 4 * w + 3) << 24;
}

// ---- CRC-32 -----------------------------------------------------------------------------------------------------------------------
TP_RULE inline uint32_t crc_table_entry(uint32_t i)
{
	uint32_t c = i;
	for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
	return c;
}
// CRC-32 of in[from, to) as gzip defines it; 0 for no bytes
TP_RULE inline uint32_t crc_bytes(const uint32_t* table, const unsigned char* in, uint32_t from, uint32_t to)
{
	uint32_t c = 0xFFFFFFFFu;
	for (uint32_t p = from; p < to; p++) c = table[(c ^ in[p]) & 0xFF] ^ (c >> 8);
	return c ^ 0xFFFFFFFFu;
}
// a(x) * b(x) modulo the polynomial, both reflected (bit 31 = x^0)
TP_RULE inline uint32_t crc_multiply(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 0x80000000u; m != 0; m >>= 1) {
		if (a & m) p ^= b;
		b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
	}
	return p;
}
// x^(8 * nbytes) modulo the polynomial
TP_RULE inline uint32_t crc_shift(uint64_t nbytes)
{
	uint32_t r = 0x80000000u, b = 0x00800000u;                 // x^0, x^8
	for (; nbytes; nbytes >>= 1) {
		if (nbytes & 1) r = crc_multiply(r, b);
		b = crc_multiply(b, b);
	}
	return r;
}
// crc(A || B) from crc(A), crc(B) and len(B)
TP_RULE inline uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc_multiply(crc_shift(len_b), crc_a) ^ crc_b; }
// A chunk's CRC from 64 slices: lane l takes the bytes [slice_begin(l), slice_begin(l + 1)); the chunk's CRC is the exclusive or of
// the lanes' crc_slice_term -- the combine operator is linear.
TP_RULE inline uint32_t slice_begin(uint32_t n, int lane) { const uint32_t per = (n + kLanes - 1) / kLanes, at = per * (uint32_t)lane; return at < n ? at : n; }
TP_RULE inline uint32_t crc_slice_term(const uint32_t* table, const unsigned char* in, uint32_t n, int lane)
{
	const uint32_t from = slice_begin(n, lane), to = slice_begin(n, lane + 1);
	if (from == to) return 0;
	return crc_multiply(crc_shift(n - to), crc_bytes(table, in, from, to));
}

} // namespace tp_deflate_rules
