// deflate.hip -- batched DEFLATE (RFC 1951) on the device: the streams of a call, cut into chunks of TP_DEFLATE_CHUNK bytes with a
// window each, become byte-aligned runs of blocks that concatenate into raw deflate streams (tp_deflate), with the chunks' CRC-32
// for the gzip trailers.  What is encoded how -- matcher, codes, header, block form, CRC -- is decided by the rules of
// deflate_rules.h; this file is their parallel plumbing: ballots, prefix sums, barriers, loads and stores.
//
// tp_deflate_kernel: one wavefront (a workgroup of 64) owns a chunk from its first load to its last store.  Its steps:
//   load      the chunk into LDS, aligned words of memory as aligned words of LDS
//   checksum  64 slice CRCs, shifted to their place by the combine operator and folded with exclusive or
//   parse     groups of 64 positions, a lane each: read the hash table and count the match (hash, match), barrier, update the table
//             with an integer maximum, then the greedy parse of the group over a ballot of the lanes that hold a match; the chosen
//             lanes count their symbols in LDS and append their tokens to the chunk's token list in the work buffer (HBM: a chunk of
//             literals is 64 KiB of tokens, more than a wavefront's share of LDS)
//   build     the literal/length symbols are ranked by all lanes; lane 0 builds the three codes, the header and chooses the form
//   emit      stored: words of the stored form.  Coded: lane 0 writes the header into the LDS stage; then groups of 64 tokens, a
//             lane each: a wave-wide prefix sum of the code lengths places every token, the lanes OR their bits into the stage, and
//             the full words of the stage go out as vector stores to the chunk's pitched slot; lane 0 writes the tail
// tp_deflate_scan_kernel turns the chunk sizes into running end offsets, tp_deflate_pack_kernel moves the pitched slots to their
// place in d_out byte by byte (a chunk begins wherever the one before ended), so that nothing behind the last end is written.
#include "common.h"
#include "deflate_rules.h"

using namespace tp_deflate_rules;

namespace {

constexpr int kPackThreads = 256;
constexpr int kScanThreads = 256;

__device__ inline int wave_inclusive_sum(int v, int lane)
{
#pragma unroll
	for (int d = 1; d < kLanes; d <<= 1) {
		const int t = __shfl_up(v, d);
		if (lane >= d) v += t;
	}
	return v;
}

__device__ inline uint32_t wave_xor(uint32_t v)
{
#pragma unroll
	for (int d = 1; d < kLanes; d <<= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
	return v;
}

__device__ inline void step_load(Lds& lds, const unsigned char* src, uint32_t n, uint32_t shift, int lane)
{
	reset(lds, lane, kLanes);
	for (uint32_t w = lane; w < load_words(n, shift); w += kLanes) lds.in_words[w] = load_word(src, n, shift, w);
	__syncthreads();
}

__device__ inline uint32_t step_checksum(const Lds& lds, const unsigned char* in, uint32_t n, int lane)
{
	return wave_xor(crc_slice_term(lds.crc_table, in, n, lane));
}

// returns the number of tokens
__device__ inline uint32_t step_parse(Lds& lds, const unsigned char* in, uint32_t n, uint32_t* __restrict__ tokens, int lane)
{
	uint32_t cur = 0, n_tokens = 0;
	for (uint32_t base = 0; base < n; base += kLanes) {
		const uint32_t p = base + lane;
		const uint32_t match = (p < n && p >= cur) ? find_match(in, lds.u.hash, p, n) : 0u;
		__syncthreads();                                       // every lane has read the table
		if (p < n) hash_insert(in, lds.u.hash, p, n);
		__syncthreads();
		const uint64_t mask = __ballot((match >> 16) >= (uint32_t)kMinMatch);
		const uint32_t end = base + kLanes < n ? base + kLanes : n;
		uint32_t token = 0;
		bool chosen = false;
		while (cur < end) {
			const int from = (int)(cur - base), ml = next_match_lane(mask, from);
			if (lane >= from && lane < ml && p < n) { chosen = true; token = literal_token(in[p]); }
			if (ml == kLanes) { cur = end; break; }
			if (lane == ml) { chosen = true; token = match_token(match); }
			cur = base + ml + ((uint32_t)__shfl((int)match, ml) >> 16);
		}
		const uint64_t chosen_mask = __ballot(chosen);
		if (chosen) {
			tokens[n_tokens + __popcll(chosen_mask & (((uint64_t)1 << lane) - 1))] = token;
			count_token(lds, token);
		}
		n_tokens += (uint32_t)__popcll(chosen_mask);
	}
	__syncthreads();
	return n_tokens;
}

__device__ inline void step_build(Lds& lds, uint32_t n, int lane)
{
	sort_symbols(lds.freq_ll, kNumLL, lds.u.b.sorted, lane, kLanes);
	__syncthreads();
	if (lane == 0) build_codes(lds, n);
	__syncthreads();
}

// the full words of the stage out to the slot, the open word to the front; returns the bits left in the stage
__device__ inline uint32_t flush_stage(Lds& lds, uint32_t at, uint32_t* __restrict__ slot, uint32_t* word_base, int lane)
{
	__syncthreads();
	const uint32_t full = at >> 5;
	for (uint32_t w = lane; w < full; w += kLanes) slot[*word_base + w] = lds.stage[w];
	const uint32_t open = lds.stage[full];
	__syncthreads();
	for (uint32_t w = lane; w <= full; w += kLanes) lds.stage[w] = 0;
	__syncthreads();
	if (lane == 0) lds.stage[0] = open;
	__syncthreads();
	*word_base += full;
	return at & 31;
}

// returns the bytes of the chunk's output
__device__ inline uint32_t step_emit(Lds& lds, const unsigned char* in, uint32_t n, const uint32_t* __restrict__ tokens, uint32_t n_tokens,
	uint32_t* __restrict__ slot, int lane)
{
	if (lds.form == kFormStored) {
		const uint32_t bytes = (uint32_t)stored_bytes(n);
		for (uint32_t w = lane; w < (bytes + 3) / 4; w += kLanes) slot[w] = stored_word(in, n, w);
		return bytes;
	}
	uint32_t word_base = 0, at = 0;
	if (lane == 0) at = put_header(lds);
	at = (uint32_t)__shfl((int)at, 0);
	at = flush_stage(lds, at, slot, &word_base, lane);
	for (uint32_t t0 = 0; t0 < n_tokens; t0 += kLanes) {
		int nbits = 0;
		uint64_t bits = 0;
		if (t0 + lane < n_tokens) bits = token_bits(lds, tokens[t0 + lane], &nbits);
		const int behind = wave_inclusive_sum(nbits, lane);
		or_bits(lds.stage, at + (uint32_t)(behind - nbits), bits, nbits);
		at += (uint32_t)__shfl(behind, kLanes - 1);
		at = flush_stage(lds, at, slot, &word_base, lane);
	}
	if (lane == 0) at = put_tail(lds, at);
	at = (uint32_t)__shfl((int)at, 0);
	__syncthreads();
	for (uint32_t w = lane; w < (at + 31) / 32; w += kLanes) slot[word_base + w] = lds.stage[w];
	return word_base * 4 + at / 8;
}

__global__ void __launch_bounds__(kLanes) tp_deflate_kernel(const unsigned char* __restrict__ d_in, const ChunkDesc* __restrict__ table, uint32_t* __restrict__ tokens_all,
	uint32_t* __restrict__ slots_all, uint32_t* __restrict__ sizes, uint32_t* __restrict__ crcs)
{
	__shared__ Lds lds;
	const int lane = threadIdx.x;
	const uint64_t c = blockIdx.x;
	const unsigned char* src = d_in + table[c].offset;
	const uint32_t n = table[c].nbytes;
	const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3);
	uint32_t* tokens = tokens_all + c * (uint64_t)kChunk;
	uint32_t* slot = slots_all + c * (uint64_t)(kSlotBytes / 4);

	step_load(lds, src, n, shift, lane);
	const unsigned char* in = input_of(lds, shift);
	const uint32_t crc = step_checksum(lds, in, n, lane);
	const uint32_t n_tokens = step_parse(lds, in, n, tokens, lane);
	step_build(lds, n, lane);
	const uint32_t bytes = step_emit(lds, in, n, tokens, n_tokens, slot, lane);
	if (lane == 0) {
		sizes[c] = bytes;
		crcs[c] = crc;
	}
}

// running end offsets of the chunks: one workgroup, a contiguous piece of the sizes per thread
__global__ void __launch_bounds__(kScanThreads) tp_deflate_scan_kernel(const uint32_t* __restrict__ sizes, uint64_t* __restrict__ ends, uint64_t n)
{
	__shared__ uint64_t piece[kScanThreads];
	const uint64_t per = (n + kScanThreads - 1) / kScanThreads;
	const uint64_t from = per * threadIdx.x < n ? per * threadIdx.x : n, to = from + per < n ? from + per : n;
	uint64_t sum = 0;
	for (uint64_t c = from; c < to; c++) sum += sizes[c];
	piece[threadIdx.x] = sum;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t run = 0;
		for (int t = 0; t < kScanThreads; t++) { const uint64_t s = piece[t]; piece[t] = run; run += s; }
	}
	__syncthreads();
	uint64_t run = piece[threadIdx.x];
	for (uint64_t c = from; c < to; c++) { run += sizes[c]; ends[c] = run; }
}

__global__ void __launch_bounds__(kPackThreads) tp_deflate_pack_kernel(const unsigned char* __restrict__ slots, const uint32_t* __restrict__ sizes,
	const uint64_t* __restrict__ ends, unsigned char* __restrict__ d_out)
{
	const uint64_t c = blockIdx.x;
	const uint32_t bytes = sizes[c];
	const unsigned char* src = slots + c * (uint64_t)kSlotBytes;
	unsigned char* dst = d_out + (ends[c] - bytes);
	for (uint32_t k = threadIdx.x; k < bytes; k += kPackThreads) dst[k] = src[k];
}

} // namespace

extern "C" uint64_t tp_deflate_chunk_bytes(void) { return (uint64_t)kChunk; }

extern "C" uint64_t tp_deflate_bound(uint64_t nbytes) { return bound_of(nbytes); }

extern "C" uint64_t tp_deflate_work_bytes(const uint64_t* h_stream_offsets, int64_t n_streams)
{
	if (h_stream_offsets == nullptr || n_streams < 1) return 0;
	uint64_t chunks = 0;
	for (int64_t s = 0; s < n_streams; s++) {
		if (h_stream_offsets[s + 1] < h_stream_offsets[s]) return 0;
		chunks += n_chunks_of(h_stream_offsets[s + 1] - h_stream_offsets[s]);
	}
	return work_layout(chunks).total;
}

extern "C" uint32_t tp_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc_combine(crc_a, crc_b, len_b); }

extern "C" int tp_deflate(tp_ctx* ctx, const void* d_in, const uint64_t* h_stream_offsets, int64_t n_streams, void* d_out, uint64_t out_capacity,
	uint64_t* d_chunk_end, uint32_t* d_chunk_crc, void* d_work, uint64_t work_bytes)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	uint64_t n_chunks = 0;
	const char* msg = check(reinterpret_cast<uintptr_t>(d_in), h_stream_offsets, n_streams, reinterpret_cast<uintptr_t>(d_out), out_capacity,
		reinterpret_cast<uintptr_t>(d_chunk_end), reinterpret_cast<uintptr_t>(d_chunk_crc), reinterpret_cast<uintptr_t>(d_work), work_bytes, &n_chunks);
	TP_REQUIRE(ctx, msg == nullptr, msg);
	if (n_chunks == 0) return TP_OK;
	std::vector<ChunkDesc> table((size_t)n_chunks);
	chunk_table(h_stream_offsets, n_streams, table.data());
	const WorkLayout lay = work_layout(n_chunks);
	unsigned char* work = static_cast<unsigned char*>(d_work);
	int rc = tp_memcpy_h2d(ctx, work + lay.table, table.data(), n_chunks * sizeof(ChunkDesc));
	if (rc != TP_OK) return rc;
	uint32_t* sizes = reinterpret_cast<uint32_t*>(work + lay.sizes);
	TP_LAUNCH(ctx, TPK_DEFLATE, tp_deflate_kernel, dim3((unsigned)n_chunks), dim3(kLanes), 0, static_cast<const unsigned char*>(d_in),
		reinterpret_cast<const ChunkDesc*>(work + lay.table), reinterpret_cast<uint32_t*>(work + lay.tokens), reinterpret_cast<uint32_t*>(work + lay.slots), sizes, d_chunk_crc);
	TP_LAUNCH_CHECK(ctx, "tp_deflate_kernel");
	TP_LAUNCH(ctx, TPK_DEFLATE_SCAN, tp_deflate_scan_kernel, dim3(1), dim3(kScanThreads), 0, static_cast<const uint32_t*>(sizes), d_chunk_end, n_chunks);
	TP_LAUNCH_CHECK(ctx, "tp_deflate_scan_kernel");
	TP_LAUNCH(ctx, TPK_DEFLATE_PACK, tp_deflate_pack_kernel, dim3((unsigned)n_chunks), dim3(kPackThreads), 0, static_cast<const unsigned char*>(work + lay.slots),
		static_cast<const uint32_t*>(sizes), static_cast<const uint64_t*>(d_chunk_end), static_cast<unsigned char*>(d_out));
	TP_LAUNCH_CHECK(ctx, "tp_deflate_pack_kernel");
	return TP_OK;
	TP_API_END(ctx)
}
