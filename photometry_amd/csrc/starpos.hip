// starpos.hip -- the positions a LinPSF fit takes for the stars of many targets that each move by a series of their own
// (tp_star_positions_targets): a group of target pixel files, where POS_CORR1/2 is per file.  For star s of target t at cadence k
//   d_pos[s][k] = (double)(d_base[s] + (float)d_shift[t][j]),  j = d_lookup[t][k] or k,
// which is the plugin's `cat['row_stamp'] + np.float32(jit[k, 1])` (catalog_attime for a source with `jitter`) widened as
// do_photometry widens it.  tp_star_positions (linpsf.hip) is the same for ONE series shared by all stars -- a CCD region.
// What is decided -- checks, grid, lookup, arithmetic, offsets -- is starpos_rules.h; this file is the parallel plumbing.
//
// A thread owns one cadence, a block 256 consecutive ones; blockIdx.y walks the stars.  Per star a block reads 256 consecutive
// doubles of its target's series (the stars of a target read the same lines: they come out of L2) and stores 256 consecutive
// doubles of the star's row; all offsets are 64-bit.  Nothing beyond n_cad is written.
#include "common.h"
#include "starpos_rules.h"

using namespace tp_starpos;

namespace {

__global__ __launch_bounds__(kThreads) void tp_star_positions_targets_kernel(int64_t n_stars, int32_t n_cad, const float* __restrict__ base,
	const int32_t* __restrict__ star_target, const double* __restrict__ shift, int64_t shift_pitch, const int32_t* __restrict__ lookup, int64_t lookup_pitch,
	int32_t n_targets, double* __restrict__ pos, int64_t pos_pitch)
{
	const int64_t k = cadence_of(blockIdx.x, threadIdx.x);
	if (k >= n_cad) return;
	for (int64_t s = blockIdx.y; s < n_stars; s += gridDim.y)
		pos[pos_index(s, k, pos_pitch)] = star_position(base, star_target, shift, shift_pitch, lookup, lookup_pitch, n_targets, s, k);
}

} // namespace

extern "C" int tp_star_positions_targets(tp_ctx* ctx, int64_t n_stars, int32_t n_cad, const float* d_base, const int32_t* d_star_target,
	const double* d_shift, int64_t shift_pitch, const int32_t* d_lookup, int64_t lookup_pitch, int32_t n_targets, double* d_pos, int64_t pos_pitch)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const char* msg = sizes_check(n_stars, n_cad, n_targets, shift_pitch, d_lookup != nullptr, lookup_pitch, pos_pitch);
	TP_REQUIRE(ctx, msg == nullptr, msg);
	if (n_stars == 0 || n_cad == 0) return TP_OK;
	msg = pointers_check(reinterpret_cast<uintptr_t>(d_base), reinterpret_cast<uintptr_t>(d_star_target), reinterpret_cast<uintptr_t>(d_shift),
		reinterpret_cast<uintptr_t>(d_pos));
	TP_REQUIRE(ctx, msg == nullptr, msg);
	TP_LAUNCH(ctx, TPK_STAR_POSITIONS_TARGETS, tp_star_positions_targets_kernel, dim3((unsigned)blocks_x(n_cad), (unsigned)blocks_y(n_stars)), dim3(kThreads), 0,
		n_stars, n_cad, d_base, d_star_target, d_shift, shift_pitch, d_lookup, lookup_pitch, n_targets, d_pos, pos_pitch);
	TP_LAUNCH_CHECK(ctx, "tp_star_positions_targets_kernel");
	return TP_OK;
	TP_API_END(ctx)
}
