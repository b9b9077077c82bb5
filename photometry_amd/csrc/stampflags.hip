// stampflags.hip -- the per-stamp flag series (tp_stamp_flag_series): for every target of a batch and every frame of the region's
// pixel-flag stack, whether any pixel of the target's stamp carries one of the bits of a mask.  It is what save_lightcurve does on the
// host in the reference, one target at a time -- `np.any(self.pixelflags_cube & PixelQualityFlags.BackgroundShenanigans != 0, axis=(0, 1))`
// becomes CorrectorQualityFlags.BackgroundShenanigans in the QUALITY column (BasePhotometry.py:1445-1449) -- for the whole batch in one
// launch on the stack as prepare.prepare_frames leaves it in HBM: uint8 [T][R][C].  The decisions -- argument checks, the stamps
// relative to the frames, grid, lane map, addresses -- are the rules of stampflags_rules.h; this file is their parallel plumbing.
//
// A wavefront owns one target and kTileT = 16 consecutive frames.  It lies over the stamp as 4 rows x 16 columns of lanes (a row of
// lanes reads 16 consecutive bytes of a stamp row: a 15 x 15 stamp is 4 byte loads per lane and frame), ORs what it reads, and one
// __ballot per frame tells every lane whether any of them met the mask.  Lane k keeps the answer of frame k of the tile; after the
// last frame lanes 0 .. 15 store 16 consecutive int32 of the target's row, 64 bytes.  Stamp rows are short unaligned byte runs, each
// in a cache line of its own, so the loads are bytes: a dword load would need the frames' rows 4-byte aligned, and with an odd
// column count or frame stride they are not.
//
// The targets vary fastest over the grid: the workgroups in flight at one time read the same 16 frames, and a frame's lines come
// out of HBM once for every stamp that lies on them.  The result is integers, the same in every run.
#include "common.h"
#include "stampflags_rules.h"

using namespace tp_sflags;

namespace {

__global__ void __launch_bounds__(kThreads) tp_stamp_flags_kernel(const uint8_t* __restrict__ flags, int32_t n_frames, int32_t frame_cols, int64_t frame_stride,
	int32_t n_targets, const RelStamp* __restrict__ stamps, uint32_t flag_mask, int32_t out_value, int32_t* __restrict__ out, int64_t out_pitch, int64_t n_groups)
{
	const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
	const int64_t target = block_target(blockIdx.x, n_groups, wave);
	if (target >= n_targets) return;                       // (whole wavefronts leave: no barrier follows)
	const int64_t t0 = block_tile(blockIdx.x, n_groups) * kTileT;
	const RelStamp s = stamps[target];
	const int32_t n_row_steps = row_steps(s), n_col_steps = col_steps(s);

	int32_t mine = 0;                                      // lane k: the answer of frame t0 + k
	for (int k = 0; k < kTileT && t0 + k < n_frames; k++) {
		uint32_t seen = 0;
		for (int32_t rs = 0; rs < n_row_steps; rs++) {
			const int32_t row = lane_row(s, lane, rs);
			for (int32_t cs = 0; cs < n_col_steps; cs++) {
				const int32_t col = lane_col(s, lane, cs);
				if (in_stamp(s, row, col)) seen |= flags[flag_byte(t0 + k, frame_stride, frame_cols, row, col)];
			}
		}
		const bool any = __ballot(flagged((uint8_t)seen, flag_mask)) != 0;
		if (lane == k) mine = out_of(any, out_value);
	}
	if (lane < kTileT && t0 + lane < n_frames) out[out_index(target, t0 + lane, out_pitch)] = mine;
}

} // namespace

extern "C" int tp_stamp_flag_series(tp_ctx* ctx, const uint8_t* d_flags, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	int32_t row0, int32_t col0, int32_t n_targets, const int64_t* h_stamps, uint32_t flag_mask, int32_t out_value, int32_t* d_out, int64_t out_pitch)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const char* msg = series_check(reinterpret_cast<uintptr_t>(d_flags), n_frames, frame_rows, frame_cols, frame_stride, row0, col0, n_targets, h_stamps, flag_mask,
		reinterpret_cast<uintptr_t>(d_out), out_pitch);
	TP_REQUIRE(ctx, msg == nullptr, msg);
	std::vector<RelStamp> rel((size_t)n_targets);
	for (int64_t i = 0; i < n_targets; i++) rel[(size_t)i] = relative(h_stamps + 4 * i, row0, col0);
	// the stamps go up in one transfer; their block returns to the context's cache behind the kernel
	void* d_stamps = nullptr;
	int rc = tp_malloc(ctx, (uint64_t)n_targets * sizeof(RelStamp), &d_stamps);
	if (rc != TP_OK) return rc;
	rc = tp_memcpy_h2d(ctx, d_stamps, rel.data(), (uint64_t)n_targets * sizeof(RelStamp));
	if (rc != TP_OK) { (void)tp_free(ctx, d_stamps); return rc; }
	TP_LAUNCH(ctx, TPK_STAMP_FLAGS, tp_stamp_flags_kernel, dim3((unsigned)grid_blocks(n_frames, n_targets)), dim3(kThreads), 0, d_flags, n_frames, frame_cols,
		frame_stride, n_targets, static_cast<const RelStamp*>(d_stamps), flag_mask, out_value, d_out, out_pitch, groups_n(n_targets));
	const hipError_t launched = hipGetLastError();
	(void)tp_free(ctx, d_stamps);
	if (launched != hipSuccess) return ctx->fail(TP_ERR_HIP, "tp_stamp_flags_kernel", launched);
	return TP_OK;
	TP_API_END(ctx)
}
