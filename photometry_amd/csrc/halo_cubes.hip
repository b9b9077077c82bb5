// halo_cubes.hip -- the cubes path of Halo photometry: what halo_stack.hip does for a region's image stack, for a group of target
// pixel files that share a stamp shape and a number of cadences and nothing else.  The pixels lie in one time-fastest cube, float32
// [n_targets][height * width][t_pitch] (the pads behind n_cad are never read), and every target brings its own segments, quality
// flags and gaps: problem q = h_prob_off[i] + k is segment k of target i, so targets with one, two or more segments sit side by side.
// The host sorts every target's cadences by (segment, cadence) once (cube_lists); problem q owns the entries [lo[q], hi[q]) of its
// target's row of that list.  Time is the fast axis, so the lanes of a wavefront run along cadences wherever pixels are read:
//   stat       (4 pixels per block, one wavefront each; problem): over the problem's FITTED cadences, 64 per load, the count n of
//              non-NaN values, the count c of values < minflux, a = max{x < minflux}, b = min{x >= minflux} (keys) -- per lane
//              over the tiles, then across the wavefront: integer sums, max and min, all order-independent -- and the pixel
//              decision drop_pixel from them.  A segment without a cadence has n = 0: every mask pixel is kept;
//   cad        (256 cadences per block; problem): lane = cadence, a loop over the kept pixels (their flags in LDS): the cadence is
//              kept iff every one of them is finite;
//   compact    (one block per problem): the kept pixels and cadences in ascending order, the fit flags, the counts, and the
//              position of every cadence of the target in its problem's list (-1: in none);
//   gather     (64 cadences x 64 pixels per block; problem): the transposition from [pixel][time] to P[cadence][pitch] through an
//              LDS tile of pitch 65 -- rows of 64 consecutive cadences in, rows of 64 consecutive pixels out, both sides coalesced
//              and free of bank conflicts, as in tpfin.hip -- and the concatenated fit bytes;
//   norm       (one block per problem): numpy's median of l over the fitted cadences and the weight map w / median;
//   lightcurve (256 cadences per block; target): lane = cadence: corr_flux, flux, and flux_err as a loop over the stamp's pixels in
//              ascending order (NaN terms count as 0) in the grouping of numpy's pairwise sum -- the same chains for a cadence
//              whatever the batch, and the bits of the per-file path's np.nansum.
// The pixel and cadence rules, the keys and the host tables with their checks are halo_rules.h; rank and selection are halo_dev.h.
// No float atomics and no atomics on global memory at all: a target gives the same bits alone, in a batch and in any chunking.
#include "halo_dev.h"

namespace {

using namespace tp_halo;

constexpr int kWaves = kThreads / 64;
constexpr int kTileC = 64, kTileP = 64, kTilePitch = 65;   // the gather tile: cadences x pixels, LDS pitch in dwords

// pixkeep uint8 [n_prob][HW]
__global__ __launch_bounds__(kThreads) void tp_halo_cube_stat_kernel(CubeGeom g, const float* __restrict__ images, const uint8_t* __restrict__ mask,
	const int32_t* __restrict__ cadlist, const uint8_t* __restrict__ fitlist, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
	const int32_t* __restrict__ target, double minflux, uint8_t* pixkeep)
{
	const int q = blockIdx.y, i = target[q];
	const int HW = g.height * g.width;
	const int lane = threadIdx.x & 63;
	const int p = blockIdx.x * kWaves + (threadIdx.x >> 6);        // (one pixel per wavefront: what follows is uniform in it)
	if (p >= HW) return;
	const int64_t s = (int64_t)q * HW + p;
	if (!mask[(int64_t)i * HW + p]) {
		if (lane == 0) pixkeep[s] = 0;
		return;
	}
	const float* series = images + cube_offset(g, i, p);
	const int32_t* cl = cadlist + (int64_t)i * g.n_cad;
	const uint8_t* fl = fitlist + (int64_t)i * g.n_cad;
	int32_t n = 0, c = 0;
	uint32_t ak = 0u, bk = 0xffffffffu;
	const int j1 = hi[q];
	for (int j = lo[q] + lane; j < j1; j += 64) {
		if (!fl[j]) continue;
		const float x = series[cl[j]];
		if (x != x) continue;
		n++;
		const uint32_t key = fkey(x);
		if ((double)x < minflux) { c++; ak = max(ak, key); }
		else bk = min(bk, key);
	}
	for (int o = 32; o >= 1; o >>= 1) {
		n += __shfl_xor(n, o, 64);
		c += __shfl_xor(c, o, 64);
		ak = max(ak, (uint32_t)__shfl_xor((int)ak, o, 64));
		bk = min(bk, (uint32_t)__shfl_xor((int)bk, o, 64));
	}
	if (lane == 0) pixkeep[s] = drop_pixel(n, c, ak, bk, minflux) ? 0 : 1;
}

// cadkeep uint8 [n_prob][n_cad], indexed by the position in the problem's part of cadlist (j - lo[q])
__global__ __launch_bounds__(kThreads) void tp_halo_cube_cad_kernel(CubeGeom g, const float* __restrict__ images, const int32_t* __restrict__ cadlist,
	const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, const int32_t* __restrict__ target, const uint8_t* __restrict__ pixkeep,
	uint8_t* cadkeep)
{
	__shared__ uint8_t keep[kMaxStamp];
	const int q = blockIdx.y, i = target[q];
	const int HW = g.height * g.width;
	const int first = lo[q], count = hi[q] - first;
	const int j0 = blockIdx.x * kThreads;
	if (j0 >= count) return;                                       // (the whole block)
	for (int p = threadIdx.x; p < HW; p += kThreads) keep[p] = pixkeep[(int64_t)q * HW + p];
	__syncthreads();
	const int j = j0 + threadIdx.x;
	if (j >= count) return;
	const int t = cadlist[(int64_t)i * g.n_cad + first + j];
	const float* at = images + cube_offset(g, i, 0) + t;
	bool bad = false;
	for (int p = 0; p < HW; p++)
		if (keep[p]) bad |= !pixel_finite(at[(int64_t)p * g.t_pitch]);
	cadkeep[(int64_t)q * g.n_cad + j] = bad ? 0 : 1;
}

// ascending list of the set flags: emit(index, flag, rank among the set ones); returns the count (every thread)
template <class F> __device__ int compact_block(const uint8_t* flags, int n, int* wcount, F&& emit) {
	int base = 0;
	for (int c0 = 0; c0 < n; c0 += kThreads) {
		const int t = c0 + threadIdx.x;
		const bool flag = t < n && flags[t] != 0;
		int total;
		const int before = block_rank<kThreads>(flag, wcount, total);
		emit(t, flag, base + before);
		base += total;
		__syncthreads();
	}
	return base;
}

// pix int32 [n_prob][HW], cad int32 [n_prob][n_cad], fit uint8 [n_prob][n_cad], cadpos int32 [n_targets][n_cad] (preset to -1)
__global__ __launch_bounds__(kThreads) void tp_halo_cube_compact_kernel(CubeGeom g, const int32_t* __restrict__ cadlist, const uint8_t* __restrict__ fitlist,
	const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, const int32_t* __restrict__ target, const uint8_t* __restrict__ pixkeep,
	const uint8_t* __restrict__ cadkeep, int32_t* pix, int32_t* cad, uint8_t* fit, int32_t* cadpos, int32_t* npix, int32_t* ncad)
{
	__shared__ int wcount[kWaves];
	const int64_t q = blockIdx.x;
	const int i = target[q];
	const int HW = g.height * g.width, T = g.n_cad;
	const int first = lo[q], count = hi[q] - first;
	int32_t* mypix = pix + q * HW;
	const int np = compact_block(pixkeep + q * HW, HW, wcount, [&](int t, bool flag, int rank) { if (flag) mypix[rank] = t; });
	const int32_t* cl = cadlist + (int64_t)i * T + first;
	const uint8_t* fl = fitlist + (int64_t)i * T + first;
	int32_t* mycad = cad + q * T;
	uint8_t* myfit = fit + q * T;
	int32_t* mypos = cadpos + (int64_t)i * T;
	const int nc = compact_block(cadkeep + q * T, count, wcount, [&](int t, bool flag, int rank) {
		if (flag) {
			const int c = cl[t];
			mycad[rank] = c;
			myfit[rank] = fl[t];
			mypos[c] = rank;
		}
	});
	if (threadIdx.x == 0) {
		npix[q] = np;
		ncad[q] = nc;
	}
}

__global__ __launch_bounds__(kThreads) void tp_halo_cube_gather_kernel(CubeGeom g, const float* __restrict__ images, const GatherProb* __restrict__ probs,
	const int32_t* __restrict__ target, const int32_t* __restrict__ pix, const int32_t* __restrict__ cad, const uint8_t* __restrict__ fit,
	float* P, uint8_t* fit_out)
{
	__shared__ float tile[kTileP * kTilePitch];
	const GatherProb pr = probs[blockIdx.z];
	const int r0 = blockIdx.x * kTileC, p0 = blockIdx.y * kTileP;
	if (r0 >= pr.ncad || p0 >= pr.pitch) return;                   // (the whole block)
	const int HW = g.height * g.width;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int32_t* mypix = pix + (int64_t)pr.q * HW;
	const int32_t* mycad = cad + (int64_t)pr.q * g.n_cad;
	const float* cube = images + cube_offset(g, target[pr.q], 0);
	// in: row pp of the tile is 64 consecutive kept cadences of one kept pixel
	const int r = r0 + lane;
	const int t = r < pr.ncad ? mycad[r] : -1;
	for (int pp = wave; pp < kTileP; pp += kWaves) {
		const int p = p0 + pp;
		if (p < pr.npix && t >= 0) tile[pp * kTilePitch + lane] = cube[(int64_t)mypix[p] * g.t_pitch + t];
	}
	__syncthreads();
	// out: row tt of the tile's transpose is 64 consecutive pixels of one row of P; zeros in the padding of the row
	const int p = p0 + lane;
	for (int tt = wave; tt < kTileC; tt += kWaves) {
		const int row = r0 + tt;
		if (row < pr.ncad && p < pr.pitch) P[pr.p_off + (int64_t)row * pr.pitch + p] = p < pr.npix ? tile[lane * kTilePitch + tt] : 0.0f;
	}
	if (blockIdx.y == 0 && threadIdx.x < kTileC && r0 + threadIdx.x < pr.ncad)
		fit_out[pr.c_off + r0 + threadIdx.x] = fit[(int64_t)pr.q * g.n_cad + r0 + threadIdx.x];
}

// numpy's median of l over the fitted cadences of a problem: NaN for none, or for any with a NaN among them (the selection is the
// block's radix selection of halo_dev.h, the ranks and the value from the keys are halo_rules.h -- as the stack path's norm kernel)
__device__ double norm_median(const double* l, const uint8_t* fit, int ncad, int* hist, int* sh, int* cnt) {
	if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
	__syncthreads();
	int nf = 0, nn = 0;
	for (int t = threadIdx.x; t < ncad; t += kThreads)
		if (fit[t]) { nf++; nn += l[t] != l[t]; }
	if (nf) atomicAdd(&cnt[0], nf);
	if (nn) atomicAdd(&cnt[1], nn);
	__syncthreads();
	nf = cnt[0];
	nn = cnt[1];
	if (!(nf > 0 && nn == 0)) return NAN;
	auto fitted_keys = [&](auto&& visit) {
		for (int t = threadIdx.x; t < ncad; t += kThreads)
			if (fit[t]) visit(okey(l[t]));
	};
	const int k1 = mid_lo(nf), k2 = mid_hi(nf);
	const uint64_t lo = block_radix_select<kThreads>(fitted_keys, k1, hist, sh).key;
	const uint64_t hi = k2 != k1 ? block_radix_select<kThreads>(fitted_keys, k2, hist, sh).key : lo;
	return median_of_keys(lo, hi, k2 != k1);
}

// median double [n_prob] (NaN for a problem that was not run), weightmap double [n_prob][HW]; run: the run problem of q, or -1
__global__ __launch_bounds__(kThreads) void tp_halo_cube_norm_kernel(CubeGeom g, const int32_t* __restrict__ run, const NormProb* __restrict__ probs,
	const int32_t* __restrict__ pix, const uint8_t* __restrict__ fit, const double* __restrict__ w, const double* __restrict__ l,
	double* median, double* weightmap)
{
	__shared__ int hist[256];
	__shared__ int sh[2];
	__shared__ int cnt[2];
	const int64_t q = blockIdx.x;
	const int HW = g.height * g.width;
	double* wm = weightmap + q * HW;
	for (int p = threadIdx.x; p < HW; p += kThreads) wm[p] = 0.0;
	const int r = run[q];
	if (r < 0) {
		if (threadIdx.x == 0) median[q] = NAN;
		return;
	}
	const NormProb pr = probs[r];
	const double med = norm_median(l + pr.c_off, fit + pr.c_off, pr.ncad, hist, sh, cnt);
	if (threadIdx.x == 0) median[q] = med;
	__syncthreads();   // the zeros of wm before the weights
	const int32_t* mypix = pix + q * HW;
	for (int p = threadIdx.x; p < pr.npix; p += kThreads) wm[mypix[p]] = w[pr.w_off + p] / med;
}

// corr / flux / flux_err double [n_targets][n_cad]; seg int32 [n_targets][n_cad]
__global__ __launch_bounds__(kThreads) void tp_halo_cube_lightcurve_kernel(CubeGeom g, const float* __restrict__ images_err, const int32_t* __restrict__ seg,
	const int32_t* __restrict__ prob_off, const int32_t* __restrict__ run, const NormProb* __restrict__ probs, const int32_t* __restrict__ cadpos,
	const double* __restrict__ l, const int32_t* __restrict__ status, const double* __restrict__ median, const double* __restrict__ weightmap,
	const double* __restrict__ normfactor, double* corr, double* flux, double* flux_err)
{
	const int i = blockIdx.y;
	const int t = blockIdx.x * kThreads + threadIdx.x;
	if (t >= g.n_cad) return;
	const int HW = g.height * g.width;
	const int64_t o = (int64_t)i * g.n_cad + t;
	const int k = seg[o];
	if (k < 0) {
		corr[o] = NAN; flux[o] = NAN; flux_err[o] = 0.0;
		return;
	}
	const double nf = normfactor[i];
	const int64_t q = prob_off[i] + k;
	const double* wm = weightmap + q * HW;
	const float* err = images_err + cube_offset(g, i, 0) + t;
	// np.nansum(wm^2 err^2) over the stamp, the pixels in ascending order within numpy's own grouping (eight running sums per leaf of
	// 128 terms): the sum the per-file path forms on the host (halo.flux_err), bit for bit, so that a target's light-curve file is the
	// same whichever path wrote it.  A pixel without weight gives 0 or a NaN that counts as 0: its error is not read.
	const double s = lane_np_pairwise_sum([&](int p) {
		const double w2 = wm[p] * wm[p];
		if (w2 == 0.0) return 0.0;
		const double e = (double)err[(int64_t)p * g.t_pitch];
		const double term = w2 * (e * e);
		return term == term ? term : 0.0;   // nansum: a NaN term counts as 0
	}, HW);
	const int r = run[q];
	const int pos = cadpos[o];
	double c = NAN;
	if (r >= 0 && pos >= 0 && status[r] != ST_DEGENERATE) c = l[probs[r].c_off + pos] / median[q];
	corr[o] = c;
	flux[o] = c * nf;
	flux_err[o] = fabs(nf) * sqrt(s);
}

// ---- host entries ------------------------------------------------------------------------------------------------------------
template <class T> int upload(tp_ctx* ctx, T* dst, const T* src, size_t count)
{
	if (count) TP_HIP(ctx, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
	return TP_OK;
}
template <class T> int upload(tp_ctx* ctx, T* dst, const std::vector<T>& src) { return upload(ctx, dst, src.data(), src.size()); }

int cube_checks(tp_ctx* ctx, CubeGeom& g, const void* d_cube, const int32_t* h_prob_off, const int32_t* h_seg, bool with_seg)
{
	const char* bad = check_cube(g, d_cube, h_prob_off);
	if (!bad && with_seg) bad = check_cube_seg(g, h_prob_off, h_seg);
	TP_REQUIRE(ctx, !bad, bad);
	return TP_OK;
}

// target of every problem
std::vector<int32_t> targets_of(const CubeGeom& g, const int32_t* h_prob_off)
{
	std::vector<int32_t> target(g.n_prob);
	for (int i = 0; i < g.n_targets; i++)
		for (int q = h_prob_off[i]; q < h_prob_off[i + 1]; q++) target[q] = i;
	return target;
}

} // namespace

extern "C" int tp_halo_select_cubes(tp_ctx* ctx, const float* d_images, int32_t n_targets, int32_t height, int32_t width, int32_t n_cad, int32_t t_pitch,
	const uint8_t* d_mask, const int32_t* h_prob_off, const int32_t* h_seg, const int32_t* h_quality, int32_t bitmask, double minflux,
	int32_t* d_pix, int32_t* d_cad, uint8_t* d_fit, int32_t* d_cadpos, int32_t* d_npix, int32_t* d_ncad)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	CubeGeom g{n_targets, height, width, n_cad, t_pitch, 0};
	int rc = cube_checks(ctx, g, d_images, h_prob_off, h_seg, true);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, d_mask && h_quality && d_pix && d_cad && d_fit && d_cadpos && d_npix && d_ncad, "tp_halo_select_cubes: null pointer");
	// tables, uploads, launches
	const CubeLists s = cube_lists(g, h_prob_off, h_seg, h_quality, bitmask);
	const int HW = height * width;
	int32_t max_count = 0;
	for (int q = 0; q < g.n_prob; q++) max_count = std::max(max_count, s.hi[q] - s.lo[q]);
	DevBlocks dev(ctx);
	int32_t* cadlist = dev.get<int32_t>(s.cadlist.size());
	uint8_t* fitlist = dev.get<uint8_t>(s.fitlist.size());
	int32_t* lo = dev.get<int32_t>(g.n_prob);
	int32_t* hi = dev.get<int32_t>(g.n_prob);
	int32_t* target = dev.get<int32_t>(g.n_prob);
	uint8_t* pixkeep = dev.get<uint8_t>((uint64_t)g.n_prob * HW);
	uint8_t* cadkeep = dev.get<uint8_t>((uint64_t)g.n_prob * n_cad);
	if (dev.rc != TP_OK) return dev.rc;
	rc = upload(ctx, cadlist, s.cadlist);
	if (rc == TP_OK) rc = upload(ctx, fitlist, s.fitlist);
	if (rc == TP_OK) rc = upload(ctx, lo, s.lo);
	if (rc == TP_OK) rc = upload(ctx, hi, s.hi);
	if (rc == TP_OK) rc = upload(ctx, target, s.target);
	if (rc != TP_OK) return rc;
	TP_HIP(ctx, hipMemsetAsync(d_cadpos, 0xff, (size_t)n_targets * n_cad * sizeof(int32_t), ctx->stream));   // no cadence placed
	TP_LAUNCH(ctx, TPK_HALO_CUBE_STAT, tp_halo_cube_stat_kernel, dim3((unsigned)((HW + kWaves - 1) / kWaves), (unsigned)g.n_prob), dim3(kThreads), 0, g,
		d_images, d_mask, (const int32_t*)cadlist, (const uint8_t*)fitlist, (const int32_t*)lo, (const int32_t*)hi, (const int32_t*)target, minflux, pixkeep);
	TP_LAUNCH_CHECK(ctx, "tp_halo_cube_stat_kernel");
	if (max_count > 0) {
		TP_LAUNCH(ctx, TPK_HALO_CUBE_CAD, tp_halo_cube_cad_kernel, dim3((unsigned)((max_count + kThreads - 1) / kThreads), (unsigned)g.n_prob), dim3(kThreads), 0,
			g, d_images, (const int32_t*)cadlist, (const int32_t*)lo, (const int32_t*)hi, (const int32_t*)target, (const uint8_t*)pixkeep, cadkeep);
		TP_LAUNCH_CHECK(ctx, "tp_halo_cube_cad_kernel");
	}
	TP_LAUNCH(ctx, TPK_HALO_CUBE_COMPACT, tp_halo_cube_compact_kernel, dim3((unsigned)g.n_prob), dim3(kThreads), 0, g, (const int32_t*)cadlist,
		(const uint8_t*)fitlist, (const int32_t*)lo, (const int32_t*)hi, (const int32_t*)target, (const uint8_t*)pixkeep, (const uint8_t*)cadkeep, d_pix, d_cad,
		d_fit, d_cadpos, d_npix, d_ncad);
	TP_LAUNCH_CHECK(ctx, "tp_halo_cube_compact_kernel");
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host vectors the asynchronous copies read must outlive them
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_halo_gather_cubes(tp_ctx* ctx, const float* d_images, int32_t n_targets, int32_t height, int32_t width, int32_t n_cad, int32_t t_pitch,
	const int32_t* h_prob_off, const int32_t* d_pix, const int32_t* d_cad, const uint8_t* d_fit, int32_t n_run, const int32_t* h_index,
	const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad, float* d_P, uint8_t* d_fit_out)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	CubeGeom g{n_targets, height, width, n_cad, t_pitch, 0};
	int rc = cube_checks(ctx, g, d_images, h_prob_off, nullptr, false);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, n_run >= 0 && n_run <= 65535, "tp_halo_gather_cubes: 0 .. 65535 problems per call");
	if (n_run == 0) return TP_OK;
	TP_REQUIRE(ctx, d_pix && d_cad && d_fit && h_index && h_p_offset && h_npix && h_ncad && d_P && d_fit_out, "tp_halo_gather_cubes: null pointer");
	std::vector<GatherProb> probs;
	int32_t max_ncad = 0, max_pitch = 0;
	const char* bad = check_cube_gather(g, n_run, h_index, h_p_offset, h_npix, h_ncad, probs, max_ncad, max_pitch);
	TP_REQUIRE(ctx, !bad, bad);
	if (max_ncad == 0) return TP_OK;
	const std::vector<int32_t> target = targets_of(g, h_prob_off);
	DevBlocks dev(ctx);
	GatherProb* dprobs = dev.get<GatherProb>(n_run);
	int32_t* dtarget = dev.get<int32_t>(target.size());
	if (dev.rc != TP_OK) return dev.rc;
	rc = upload(ctx, dprobs, probs);
	if (rc == TP_OK) rc = upload(ctx, dtarget, target);
	if (rc != TP_OK) return rc;
	const dim3 grid((unsigned)((max_ncad + kTileC - 1) / kTileC), (unsigned)((max_pitch + kTileP - 1) / kTileP), (unsigned)n_run);
	TP_LAUNCH(ctx, TPK_HALO_CUBE_GATHER, tp_halo_cube_gather_kernel, grid, dim3(kThreads), 0, g, d_images, (const GatherProb*)dprobs, (const int32_t*)dtarget,
		d_pix, d_cad, d_fit, d_P, d_fit_out);
	TP_LAUNCH_CHECK(ctx, "tp_halo_cube_gather_kernel");
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_halo_outputs_cubes(tp_ctx* ctx, const float* d_images_err, int32_t n_targets, int32_t height, int32_t width, int32_t n_cad, int32_t t_pitch,
	const int32_t* h_prob_off, const int32_t* h_seg, const int32_t* d_pix, const int32_t* d_cadpos, int32_t n_run, const int32_t* h_index,
	const int32_t* h_npix, const int32_t* h_ncad, const uint8_t* d_fit, const double* d_w, const double* d_l, const int32_t* d_status,
	const double* h_normfactor, double* d_median, double* d_corr, double* d_flux, double* d_flux_err, double* d_weightmap)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	CubeGeom g{n_targets, height, width, n_cad, t_pitch, 0};
	int rc = cube_checks(ctx, g, d_images_err, h_prob_off, h_seg, true);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, n_run >= 0 && n_run <= 65535, "tp_halo_outputs_cubes: 0 .. 65535 problems per call");
	TP_REQUIRE(ctx, d_pix && d_cadpos && h_normfactor && d_median && d_corr && d_flux && d_flux_err && d_weightmap, "tp_halo_outputs_cubes: null pointer");
	TP_REQUIRE(ctx, n_run == 0 || (h_index && h_npix && h_ncad && d_fit && d_w && d_l && d_status), "tp_halo_outputs_cubes: null pointer");
	// tables, uploads, launches
	std::vector<NormProb> probs;
	std::vector<int32_t> run;
	const char* bad = check_cube_norm(g, n_run, h_index, h_npix, h_ncad, probs, run);
	TP_REQUIRE(ctx, !bad, bad);
	DevBlocks dev(ctx);
	NormProb* dprobs = dev.get<NormProb>(probs.size());
	int32_t* drun = dev.get<int32_t>(run.size());
	int32_t* dseg = dev.get<int32_t>((uint64_t)n_targets * n_cad);
	int32_t* doff = dev.get<int32_t>((uint64_t)n_targets + 1);
	double* dnorm = dev.get<double>(n_targets);
	if (dev.rc != TP_OK) return dev.rc;
	rc = upload(ctx, dprobs, probs);
	if (rc == TP_OK) rc = upload(ctx, drun, run);
	if (rc == TP_OK) rc = upload(ctx, dseg, h_seg, (size_t)n_targets * n_cad);
	if (rc == TP_OK) rc = upload(ctx, doff, h_prob_off, (size_t)n_targets + 1);
	if (rc == TP_OK) rc = upload(ctx, dnorm, h_normfactor, (size_t)n_targets);
	if (rc != TP_OK) return rc;
	TP_LAUNCH(ctx, TPK_HALO_CUBE_NORM, tp_halo_cube_norm_kernel, dim3((unsigned)g.n_prob), dim3(kThreads), 0, g, (const int32_t*)drun, (const NormProb*)dprobs,
		d_pix, d_fit, d_w, d_l, d_median, d_weightmap);
	TP_LAUNCH_CHECK(ctx, "tp_halo_cube_norm_kernel");
	TP_LAUNCH(ctx, TPK_HALO_CUBE_LIGHTCURVE, tp_halo_cube_lightcurve_kernel, dim3((unsigned)((n_cad + kThreads - 1) / kThreads), (unsigned)n_targets), dim3(kThreads),
		0, g, d_images_err, (const int32_t*)dseg, (const int32_t*)doff, (const int32_t*)drun, (const NormProb*)dprobs, d_cadpos, d_l, d_status,
		(const double*)d_median, (const double*)d_weightmap, (const double*)dnorm, d_corr, d_flux, d_flux_err);
	TP_LAUNCH_CHECK(ctx, "tp_halo_cube_lightcurve_kernel");
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return TP_OK;
	TP_API_END(ctx)
}
