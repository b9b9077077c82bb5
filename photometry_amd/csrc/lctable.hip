// lctable.hip -- the data unit of the LIGHTCURVE binary table of a light-curve file (FILEVER 1.5, lcfile.py) written on the device from
// the struct-of-arrays planes a run holds -- time, timecorr, cadenceno, the five light-curve planes, QUALITY, pixel quality, pos_corr --
// with its DATASUM (tp_lc_table_pack), and a batched copy of byte ranges that puts the host-built pieces of a window of files beside
// them (tp_lc_place).  On the host this is the recarray fill, `tobytes`, the pad and `_sum32` of fitsio.bintable_hdu.  The decisions --
// row layout, conversions, word sum, pad, tile geometry, LDS index, refusals -- are the rules of lctable_rules.h; this file is their
// parallel plumbing.
//
// A wavefront owns a tile of 64 rows of one target; a workgroup is four of them.  Lane l loads the 14 values of row l: along a column
// the lanes read consecutive cadences (512 or 256 contiguous bytes; the kept-row list skips the dropped ones), swaps them in
// registers and writes the row as six 16-byte pieces into the wavefront's LDS tile (pitch 28 words: lctable_rules.h).  After the
// barrier lane l stores pieces l, l + 64, ... of the tile: every store instruction of a wavefront is 1 KiB of the data unit in a
// line.  The rows behind the last one up to the next multiple of 30 are the pad: zeros, written the same way.  The word sum of a row
// comes from its native values on the way; a wavefront's sums meet by shuffles and go to the target's sum by one integer atomic, and a
// second small launch folds the carries.
//
// Traffic per row: 84 bytes read with QUALITY and pos_corr present (seven float64 and three int32 values, pos_corr's two; the vectors
// all targets share come out of the cache after the first target), 96 written.
#include "common.h"
#include "lctable_rules.h"

using namespace tp_lctable;

namespace {

__global__ void __launch_bounds__(kThreads) tp_lc_table_pack_kernel(Src src, const int32_t* __restrict__ rows, int64_t n_rows, int64_t T,
	const uint64_t* __restrict__ offsets, unsigned char* __restrict__ out, unsigned long long* __restrict__ sums, int64_t per_target)
{
	__shared__ uint4 lds[kWaves * kLdsTileWords / 4];
	const int64_t target = (int64_t)blockIdx.x / per_target;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int64_t tile = ((int64_t)blockIdx.x % per_target) * kWaves + wave;
	const int64_t padded = padded_rows(n_rows);
	const int64_t r = tile * kTileRows + lane;
	uint32_t* tl = reinterpret_cast<uint32_t*>(lds) + wave * kLdsTileWords;

	unsigned long long sum = 0;
	if (r < padded) {
		uint32_t w[kRowWords];
		if (r < n_rows) {
			const RowValues v = load_row(src, target, row_cadence(rows, r, T));
			row_words(v, w);
			sum = row_sum(v);
		} else {
#pragma unroll
			for (int k = 0; k < kRowWords; k++) w[k] = 0u;
		}
#pragma unroll
		for (int p = 0; p < kRowPieces; p++)
			*reinterpret_cast<uint4*>(tl + lds_index(lane, 4 * p)) = make_uint4(w[4 * p], w[4 * p + 1], w[4 * p + 2], w[4 * p + 3]);
	}
	__syncthreads();
	unsigned char* dst = out + offsets[target] + tile * kTileBytes;
#pragma unroll
	for (int step = 0; step < kPieceSteps; step++) {
		const Piece p = piece_of(lane, step);
		if (tile * kTileRows + p.row < padded)
			*reinterpret_cast<uint4*>(dst + p.byte) = *reinterpret_cast<const uint4*>(tl + lds_index(p.row, p.word));
	}
	for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
	if (lane == 0 && tile * kTileRows < n_rows) atomicAdd(sums + target, sum);
}

__global__ void tp_lc_table_fold_kernel(unsigned long long* sums, int64_t n)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) sums[i] = fold32(sums[i]);
}

// thread g moves the g-th 16-byte piece of the call; table: first[n + 1], then src_offset[n], then dst_offset[n]
__global__ void __launch_bounds__(kThreads) tp_lc_place_kernel(const unsigned char* __restrict__ src, const uint64_t* __restrict__ table, int64_t n_segments,
	unsigned char* __restrict__ dst, uint64_t n_pieces)
{
	const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
	if (g >= n_pieces) return;
	const int64_t k = segment_of(table, n_segments, g);
	const uint64_t within = 16 * (g - table[k]);
	*reinterpret_cast<uint4*>(dst + table[2 * n_segments + 1 + k] + within) = *reinterpret_cast<const uint4*>(src + table[n_segments + 1 + k] + within);
}

// a small host table into a block of the context's cache, by the library's small-transfer path
int upload_table(tp_ctx* ctx, const uint64_t* h, size_t n, void** d)
{
	int rc = tp_malloc(ctx, n * sizeof(uint64_t), d);
	if (rc != TP_OK) return rc;
	rc = tp_memcpy_h2d(ctx, *d, h, n * sizeof(uint64_t));
	if (rc != TP_OK) { (void)tp_free(ctx, *d); *d = nullptr; }
	return rc;
}

} // namespace

extern "C" int tp_lc_table_pack(tp_ctx* ctx, const tp_lc_table_src* h_src, const int32_t* d_rows, int64_t n_rows, int64_t T, int32_t n_targets, void* d_out,
	const uint64_t* h_out_offsets, uint64_t out_capacity, uint64_t* d_datasum)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	Src src{};
	if (h_src != nullptr) {
		src.time = reinterpret_cast<const uint64_t*>(h_src->time); src.time_stride = h_src->time_stride;
		src.timecorr = reinterpret_cast<const uint64_t*>(h_src->timecorr); src.timecorr_stride = h_src->timecorr_stride;
		src.cadenceno = h_src->cadenceno; src.cadenceno_stride = h_src->cadenceno_stride;
		src.pixel_quality = h_src->pixel_quality; src.pixel_quality_stride = h_src->pixel_quality_stride;
		src.lc = reinterpret_cast<const uint64_t*>(h_src->lc); src.lc_plane_stride = h_src->lc_plane_stride; src.lc_target_stride = h_src->lc_target_stride;
		src.quality = h_src->quality; src.quality_stride = h_src->quality_stride;
		src.pos_corr = reinterpret_cast<const uint64_t*>(h_src->pos_corr); src.pos_corr_stride = h_src->pos_corr_stride;
	}
	const char* msg = pack_check(h_src ? &src : nullptr, reinterpret_cast<uintptr_t>(d_rows), n_rows, T, n_targets, reinterpret_cast<uintptr_t>(d_out), h_out_offsets,
		out_capacity, reinterpret_cast<uintptr_t>(d_datasum));
	TP_REQUIRE(ctx, msg == nullptr, msg);
	unsigned long long* sums = reinterpret_cast<unsigned long long*>(d_datasum);
	TP_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)n_targets * sizeof(unsigned long long), ctx->stream));
	if (n_rows == 0) return TP_OK;
	void* d_offsets = nullptr;
	int rc = upload_table(ctx, h_out_offsets, (size_t)n_targets, &d_offsets);
	if (rc != TP_OK) return rc;
	const int64_t per_target = blocks_per_target(n_rows);
	TP_LAUNCH(ctx, TPK_LC_TABLE_PACK, tp_lc_table_pack_kernel, dim3((unsigned)(per_target * n_targets)), dim3(kThreads), 0, src, d_rows, n_rows, T,
		static_cast<const uint64_t*>(d_offsets), static_cast<unsigned char*>(d_out), sums, per_target);
	const hipError_t launched = hipGetLastError();
	(void)tp_free(ctx, d_offsets);
	if (launched != hipSuccess) return ctx->fail(TP_ERR_HIP, "tp_lc_table_pack_kernel", launched);
	TP_LAUNCH(ctx, TPK_LC_TABLE_FOLD, tp_lc_table_fold_kernel, dim3((unsigned)((n_targets + kThreads - 1) / kThreads)), dim3(kThreads), 0, sums, (int64_t)n_targets);
	TP_LAUNCH_CHECK(ctx, "tp_lc_table_fold_kernel");
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_lc_place(tp_ctx* ctx, const void* d_src, uint64_t src_capacity, const uint64_t* h_src_offsets, const uint64_t* h_dst_offsets, const uint64_t* h_lengths,
	int64_t n_segments, void* d_dst, uint64_t dst_capacity)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const char* msg = place_check(reinterpret_cast<uintptr_t>(d_src), src_capacity, h_src_offsets, h_dst_offsets, h_lengths, n_segments, reinterpret_cast<uintptr_t>(d_dst),
		dst_capacity);
	TP_REQUIRE(ctx, msg == nullptr, msg);
	const size_t n = (size_t)n_segments;
	std::vector<uint64_t> table(3 * n + 1);
	table[0] = 0;
	for (size_t k = 0; k < n; k++) {
		table[k + 1] = table[k] + h_lengths[k] / 16;
		table[n + 1 + k] = h_src_offsets[k];
		table[2 * n + 1 + k] = h_dst_offsets[k];
	}
	const uint64_t n_pieces = table[n];
	if (n_pieces == 0) return TP_OK;
	void* d_table = nullptr;
	int rc = upload_table(ctx, table.data(), table.size(), &d_table);
	if (rc != TP_OK) return rc;
	TP_LAUNCH(ctx, TPK_LC_PLACE, tp_lc_place_kernel, dim3((unsigned)((n_pieces + kThreads - 1) / kThreads)), dim3(kThreads), 0, static_cast<const unsigned char*>(d_src),
		static_cast<const uint64_t*>(d_table), n_segments, static_cast<unsigned char*>(d_dst), n_pieces);
	const hipError_t launched = hipGetLastError();
	(void)tp_free(ctx, d_table);
	if (launched != hipSuccess) return ctx->fail(TP_ERR_HIP, "tp_lc_place_kernel", launched);
	return TP_OK;
	TP_API_END(ctx)
}
