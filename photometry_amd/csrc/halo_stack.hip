// halo_stack.hip -- the frames path of Halo photometry: the problems of a batch of targets built on the device straight from a
// region's image stack (halo_photometry.py:118-123 the pixel mask handed in, :160-176 the segments, halophot's minflux cut and
// finite-cadence rule as restated in tests/halo_common.py::problems), and the outputs of :197-219 (normalised light curve, weight
// maps, flux error).  The solver between the two is halo.hip (tp_halo_tvmin).
//
// The stack is image-major, float32 [T][frame_rows][frame_cols]; a stamp (r1, r2, c1, c2) in CCD coordinates holds the pixels
// [r1 - row0, r2 - row0) x [c1 - col0, c2 - col0) of every frame.  Problem q = target * n_seg + segment.
//   select_stat    (cadence tile, target): per mask pixel over the tile's FITTED cadences the count of non-NaN values n, the count
//                  c of values < minflux, a = max{x < minflux}, b = min{x >= minflux}; tiles combine through integer atomics and
//                  max / min atomics on the order-preserving key of the float32 value -- all order-independent;
//   select_cad     (cadence tile, target): the pixel decision from (n, c, a, b) -- numpy's nanmedian(float64) < minflux without a
//                  sort, see drop_pixel -- then per cadence of the tile whether every kept pixel is finite;
//   select_compact (one block per problem): the kept pixels and cadences in ascending order, the fit flags, the counts, and the
//                  position of every cadence of the target in its problem's list (-1: not part of one); a segment without any
//                  cadence keeps every mask pixel (no median: NaN), as the restatement does;
//   gather         (row tile, problem): P in tp_halo_tvmin's layout and the concatenated fit bytes;
//   norm           (one block per problem): numpy's median of l over the fitted cadences (the block's radix selection on the 64-bit
//                  key, as the solver's stat kernel) and the weight map w / median placed into the stamp;
//   lightcurve     (4 cadences per block, one wave each; target): corr_flux, flux, and flux_err as a fixed-order sum over the stamp.
// The pixel and cadence rules, the keys and the host tables with their checks are halo_rules.h; rank and selection are halo_dev.h.
// No float atomics anywhere: two runs give the same bits, and a target gives the same bits alone as inside a batch.
#include "halo_dev.h"

namespace {

using namespace tp_halo;

// what a block of the two select kernels works on: segment k of target i, entries [j0, j1) of cadlist
struct SelectTile {
	int i, k, j0, j1, HW;
	int64_t frame, nstat, q;
	const int32_t* st;
};
__device__ SelectTile select_tile(const StackGeom& g, const int32_t* stamps, const int32_t* tiles) {
	SelectTile t;
	t.i = blockIdx.y;
	t.k = tiles[3 * blockIdx.x]; t.j0 = tiles[3 * blockIdx.x + 1]; t.j1 = tiles[3 * blockIdx.x + 2];
	t.HW = g.height * g.width;
	t.frame = (int64_t)g.frame_rows * g.frame_cols;
	t.nstat = (int64_t)g.n_targets * g.n_seg * t.HW;
	t.q = (int64_t)t.i * g.n_seg + t.k;
	t.st = stamps + 4 * t.i;
	return t;
}

// tiles: int32 [n_tiles][3] = segment, first and one-past-last entry of cadlist; stats: int32 [4][n_prob * HW] = n, c, akey, bkey
__global__ __launch_bounds__(kThreads) void tp_halo_select_stat_kernel(StackGeom g, const float* __restrict__ images,
	const int32_t* __restrict__ stamps, const uint8_t* __restrict__ mask, const int32_t* __restrict__ tiles,
	const int32_t* __restrict__ cadlist, const uint8_t* __restrict__ fitlist, double minflux, int32_t* stats)
{
	const SelectTile t = select_tile(g, stamps, tiles);
	for (int p = threadIdx.x; p < t.HW; p += kThreads) {
		if (!mask[(int64_t)t.i * t.HW + p]) continue;
		const int64_t off = stamp_offset(g, t.st, p);
		int32_t n = 0, c = 0;
		uint32_t ak = 0u, bk = 0xffffffffu;
		for (int j = t.j0; j < t.j1; j++) {
			if (!fitlist[j]) continue;
			const float x = images[(int64_t)cadlist[j] * t.frame + off];
			if (x != x) continue;
			n++;
			const uint32_t key = fkey(x);
			if ((double)x < minflux) { c++; ak = max(ak, key); }
			else bk = min(bk, key);
		}
		const int64_t s = t.q * t.HW + p;
		if (n) atomicAdd(&stats[s], n);
		if (c) atomicAdd(&stats[t.nstat + s], c);
		if (ak != 0u) atomicMax(reinterpret_cast<uint32_t*>(stats) + 2 * t.nstat + s, ak);
		if (bk != 0xffffffffu) atomicMin(reinterpret_cast<uint32_t*>(stats) + 3 * t.nstat + s, bk);
	}
}

// pixkeep uint8 [n_prob][HW] (written by the first tile of every segment), cadkeep uint8 [n_prob][T] indexed by the position in the
// segment's part of cadlist (j - seg_first)
__global__ __launch_bounds__(kThreads) void tp_halo_select_cad_kernel(StackGeom g, const float* __restrict__ images,
	const int32_t* __restrict__ stamps, const uint8_t* __restrict__ mask, const int32_t* __restrict__ tiles,
	const int32_t* __restrict__ cadlist, const int32_t* __restrict__ seg_off, double minflux, const int32_t* __restrict__ stats,
	uint8_t* pixkeep, uint8_t* cadkeep)
{
	__shared__ uint8_t keep[kMaxStamp];
	__shared__ int32_t bad[kSelTile];
	const SelectTile t = select_tile(g, stamps, tiles);
	const int first = seg_off[t.k];
	for (int p = threadIdx.x; p < t.HW; p += kThreads) {
		const int64_t s = t.q * t.HW + p;
		const bool kp = mask[(int64_t)t.i * t.HW + p] != 0 &&
			!drop_pixel(stats[s], stats[t.nstat + s], (uint32_t)stats[2 * t.nstat + s], (uint32_t)stats[3 * t.nstat + s], minflux);
		keep[p] = kp;
		if (t.j0 == first) pixkeep[s] = kp;
	}
	if (threadIdx.x < kSelTile) bad[threadIdx.x] = 0;
	__syncthreads();
	for (int p = threadIdx.x; p < t.HW; p += kThreads) {
		if (!keep[p]) continue;
		const int64_t off = stamp_offset(g, t.st, p);
		for (int j = t.j0; j < t.j1; j++)
			if (!pixel_finite(images[(int64_t)cadlist[j] * t.frame + off])) bad[j - t.j0] = 1;   // (every writer stores the same value)
	}
	__syncthreads();
	for (int j = t.j0 + threadIdx.x; j < t.j1; j += kThreads) cadkeep[t.q * g.n_frames + (j - first)] = bad[j - t.j0] ? 0 : 1;
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

// pix int32 [n_prob][HW], cad int32 [n_prob][T], fit uint8 [n_prob][T], cadpos int32 [n_targets][T] (preset to -1)
__global__ __launch_bounds__(kThreads) void tp_halo_select_compact_kernel(StackGeom g, const int32_t* __restrict__ cadlist,
	const uint8_t* __restrict__ fitlist, const int32_t* __restrict__ seg_off, const uint8_t* __restrict__ mask,
	const uint8_t* __restrict__ pixkeep, const uint8_t* __restrict__ cadkeep, int32_t* pix, int32_t* cad, uint8_t* fit, int32_t* cadpos,
	int32_t* npix, int32_t* ncad)
{
	__shared__ int wcount[kThreads / 64];
	const int64_t q = blockIdx.x;
	const int i = (int)(q / g.n_seg), k = (int)(q % g.n_seg);
	const int HW = g.height * g.width;
	const int first = seg_off[k], count = seg_off[k + 1] - first;
	int32_t* mypix = pix + q * HW;
	// (a segment without a cadence has no tile that decided its pixels: no median, so every mask pixel is kept)
	const uint8_t* keep = count > 0 ? pixkeep + q * HW : mask + (int64_t)i * HW;
	const int np = compact_block(keep, HW, wcount, [&](int t, bool flag, int rank) { if (flag) mypix[rank] = t; });
	int32_t* mycad = cad + q * g.n_frames;
	uint8_t* myfit = fit + q * g.n_frames;
	int32_t* mypos = cadpos + (int64_t)i * g.n_frames;
	const int nc = compact_block(cadkeep + q * g.n_frames, count, wcount, [&](int t, bool flag, int rank) {
		if (flag) {
			const int c = cadlist[first + t];
			mycad[rank] = c;
			myfit[rank] = fitlist[first + t];
			mypos[c] = rank;
		}
	});
	if (threadIdx.x == 0) {
		npix[q] = np;
		ncad[q] = nc;
	}
}

__global__ __launch_bounds__(kThreads) void tp_halo_gather_kernel(StackGeom g, const float* __restrict__ images,
	const int32_t* __restrict__ stamps, const GatherProb* __restrict__ probs, const int32_t* __restrict__ pix,
	const int32_t* __restrict__ cad, const uint8_t* __restrict__ fit, float* P, uint8_t* fit_out)
{
	const GatherProb pr = probs[blockIdx.y];
	const int r0 = blockIdx.x * kGatherRows;
	if (r0 >= pr.ncad) return;
	const int r1 = min(r0 + kGatherRows, pr.ncad);
	const int HW = g.height * g.width;
	const int64_t frame = (int64_t)g.frame_rows * g.frame_cols;
	const int32_t* st = stamps + 4 * (pr.q / g.n_seg);
	const int32_t* mypix = pix + (int64_t)pr.q * HW;
	const int32_t* mycad = cad + (int64_t)pr.q * g.n_frames;
	for (int p = threadIdx.x; p < pr.pitch; p += kThreads) {
		const bool real = p < pr.npix;
		const int64_t off = real ? stamp_offset(g, st, mypix[p]) : 0;
		for (int r = r0; r < r1; r++)
			P[pr.p_off + (int64_t)r * pr.pitch + p] = real ? images[(int64_t)mycad[r] * frame + off] : 0.0f;
	}
	if (threadIdx.x < r1 - r0) fit_out[pr.c_off + r0 + threadIdx.x] = fit[(int64_t)pr.q * g.n_frames + r0 + threadIdx.x];
}

// numpy's median of l over the fitted cadences of a problem: NaN for none, or for any with a NaN among them
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
__global__ __launch_bounds__(kThreads) void tp_halo_norm_kernel(StackGeom g, const int32_t* __restrict__ run, const NormProb* __restrict__ probs,
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

// corr / flux / flux_err double [n_targets][T]
__global__ __launch_bounds__(kThreads) void tp_halo_lightcurve_kernel(StackGeom g, const float* __restrict__ images_err,
	const int32_t* __restrict__ stamps, const int32_t* __restrict__ seg, const int32_t* __restrict__ run, const NormProb* __restrict__ probs,
	const int32_t* __restrict__ cadpos, const double* __restrict__ l, const int32_t* __restrict__ status, const double* __restrict__ median,
	const double* __restrict__ weightmap, const double* __restrict__ normfactor, double* corr, double* flux, double* flux_err)
{
	const int i = blockIdx.y;
	const int lane = threadIdx.x & 63;
	const int t = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
	if (t >= g.n_frames) return;
	const int HW = g.height * g.width;
	const int k = seg[t];
	const double nf = normfactor[i];
	const int64_t o = (int64_t)i * g.n_frames + t;
	if (k < 0) {
		if (lane == 0) { corr[o] = NAN; flux[o] = NAN; flux_err[o] = 0.0; }
		return;
	}
	const int64_t q = (int64_t)i * g.n_seg + k;
	const int32_t* st = stamps + 4 * i;
	const double* wm = weightmap + q * HW;
	const float* err = images_err + (int64_t)t * g.frame_rows * g.frame_cols;
	// np.nansum(wm^2 err^2) over the stamp in numpy's own order: the sum the per-target path forms on the host (halo.flux_err), bit
	// for bit, so that a target's light-curve file is the same whichever path wrote it
	const double s = wave_np_pairwise_sum([&](int p) {
		const double e = (double)err[stamp_offset(g, st, p)];
		const double term = (wm[p] * wm[p]) * (e * e);
		return term == term ? term : 0.0;   // nansum: a NaN term counts as 0
	}, HW, lane);
	if (lane == 0) {
		const int r = run[q];
		const int pos = cadpos[o];
		double c = NAN;
		if (r >= 0 && pos >= 0 && status[r] != ST_DEGENERATE) c = l[probs[r].c_off + pos] / median[q];
		corr[o] = c;
		flux[o] = c * nf;
		flux_err[o] = fabs(nf) * sqrt(s);
	}
}

// ---- host entries ------------------------------------------------------------------------------------------------------------
template <class T> int upload(tp_ctx* ctx, T* dst, const T* src, size_t count)
{
	if (count) TP_HIP(ctx, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
	return TP_OK;
}
template <class T> int upload(tp_ctx* ctx, T* dst, const std::vector<T>& src) { return upload(ctx, dst, src.data(), src.size()); }

int stack_checks(tp_ctx* ctx, const StackGeom& g, const void* d_stack, const int32_t* h_stamps, const int32_t* h_seg, bool with_seg)
{
	const char* bad = stack_check(g, d_stack, h_stamps);
	if (!bad && with_seg) bad = seg_check(g, h_seg);
	TP_REQUIRE(ctx, !bad, bad);
	return TP_OK;
}

// device copies of the segment lists and the select kernels' scratch: stats, pixkeep, cadkeep
struct SelectBlocks {
	int32_t *stamps, *cadlist, *seg_off, *tiles, *stats;
	uint8_t *fitlist, *pixkeep, *cadkeep;
};

int select_uploads(tp_ctx* ctx, DevBlocks& dev, const StackGeom& g, const SegLists& s, const int32_t* h_stamps, int32_t* d_cadpos, SelectBlocks& b)
{
	const int T = g.n_frames, HW = g.height * g.width;
	const int64_t n_prob = (int64_t)g.n_targets * g.n_seg;
	b.stamps = dev.get<int32_t>((uint64_t)g.n_targets * 4);
	b.cadlist = dev.get<int32_t>(s.cadlist.size());
	b.fitlist = dev.get<uint8_t>(s.fitlist.size());
	b.seg_off = dev.get<int32_t>(s.seg_off.size());
	b.tiles = dev.get<int32_t>(s.tiles.size());
	b.stats = dev.get<int32_t>((uint64_t)n_prob * HW * 4);
	b.pixkeep = dev.get<uint8_t>((uint64_t)n_prob * HW);
	b.cadkeep = dev.get<uint8_t>((uint64_t)n_prob * T);
	if (dev.rc != TP_OK) return dev.rc;
	int rc = upload(ctx, b.stamps, h_stamps, (size_t)g.n_targets * 4);
	if (rc == TP_OK) rc = upload(ctx, b.cadlist, s.cadlist);
	if (rc == TP_OK) rc = upload(ctx, b.fitlist, s.fitlist);
	if (rc == TP_OK) rc = upload(ctx, b.tiles, s.tiles);
	if (rc == TP_OK) rc = upload(ctx, b.seg_off, s.seg_off);
	if (rc != TP_OK) return rc;
	// n, c and the largest key below start at 0, the smallest key above at all ones; no pixel kept, no cadence placed
	const size_t stat_bytes = (size_t)n_prob * HW * sizeof(int32_t);
	TP_HIP(ctx, hipMemsetAsync(b.stats, 0, 3 * stat_bytes, ctx->stream));
	TP_HIP(ctx, hipMemsetAsync(reinterpret_cast<char*>(b.stats) + 3 * stat_bytes, 0xff, stat_bytes, ctx->stream));
	TP_HIP(ctx, hipMemsetAsync(b.pixkeep, 0, (size_t)n_prob * HW, ctx->stream));
	TP_HIP(ctx, hipMemsetAsync(d_cadpos, 0xff, (size_t)g.n_targets * T * sizeof(int32_t), ctx->stream));
	return TP_OK;
}

} // namespace

extern "C" int tp_halo_select_stack(tp_ctx* ctx, const float* d_images, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int32_t row0,
	int32_t col0, int32_t n_targets, const int32_t* h_stamps, int32_t height, int32_t width, const uint8_t* d_mask, int32_t n_seg,
	const int32_t* h_seg, const int32_t* h_quality, int32_t bitmask, double minflux, int32_t* d_pix, int32_t* d_cad, uint8_t* d_fit,
	int32_t* d_cadpos, int32_t* d_npix, int32_t* d_ncad)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const StackGeom g{n_frames, frame_rows, frame_cols, row0, col0, height, width, n_seg, n_targets};
	int rc = stack_checks(ctx, g, d_images, h_stamps, h_seg, true);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, d_mask && h_quality && d_pix && d_cad && d_fit && d_cadpos && d_npix && d_ncad, "tp_halo_select_stack: null pointer");
	// tables, uploads, launches
	const SegLists s = seg_lists(n_frames, n_seg, h_seg, h_quality, bitmask);
	const unsigned n_tiles = (unsigned)(s.tiles.size() / 3);
	DevBlocks dev(ctx);
	SelectBlocks b;
	rc = select_uploads(ctx, dev, g, s, h_stamps, d_cadpos, b);
	if (rc != TP_OK) return rc;
	if (n_tiles) {
		TP_LAUNCH(ctx, TPK_HALO_SELECT_STAT, tp_halo_select_stat_kernel, dim3(n_tiles, (unsigned)n_targets), dim3(kThreads), 0, g, d_images,
			(const int32_t*)b.stamps, d_mask, (const int32_t*)b.tiles, (const int32_t*)b.cadlist, (const uint8_t*)b.fitlist, minflux, b.stats);
		TP_LAUNCH_CHECK(ctx, "tp_halo_select_stat_kernel");
		TP_LAUNCH(ctx, TPK_HALO_SELECT_CAD, tp_halo_select_cad_kernel, dim3(n_tiles, (unsigned)n_targets), dim3(kThreads), 0, g, d_images,
			(const int32_t*)b.stamps, d_mask, (const int32_t*)b.tiles, (const int32_t*)b.cadlist, (const int32_t*)b.seg_off, minflux,
			(const int32_t*)b.stats, b.pixkeep, b.cadkeep);
		TP_LAUNCH_CHECK(ctx, "tp_halo_select_cad_kernel");
	}
	TP_LAUNCH(ctx, TPK_HALO_SELECT_COMPACT, tp_halo_select_compact_kernel, dim3((unsigned)((int64_t)n_targets * n_seg)), dim3(kThreads), 0, g,
		(const int32_t*)b.cadlist, (const uint8_t*)b.fitlist, (const int32_t*)b.seg_off, d_mask, (const uint8_t*)b.pixkeep, (const uint8_t*)b.cadkeep,
		d_pix, d_cad, d_fit, d_cadpos, d_npix, d_ncad);
	TP_LAUNCH_CHECK(ctx, "tp_halo_select_compact_kernel");
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host vectors the asynchronous copies read must outlive them
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_halo_gather_stack(tp_ctx* ctx, const float* d_images, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int32_t row0,
	int32_t col0, int32_t n_targets, const int32_t* h_stamps, int32_t height, int32_t width, int32_t n_seg, const int32_t* d_pix,
	const int32_t* d_cad, const uint8_t* d_fit, int32_t n_run, const int32_t* h_index, const int64_t* h_p_offset, const int32_t* h_npix,
	const int32_t* h_ncad, float* d_P, uint8_t* d_fit_out)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const StackGeom g{n_frames, frame_rows, frame_cols, row0, col0, height, width, n_seg, n_targets};
	int rc = stack_checks(ctx, g, d_images, h_stamps, nullptr, false);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, n_run >= 0 && n_run <= 65535, "tp_halo_gather_stack: 0 .. 65535 problems per call");
	if (n_run == 0) return TP_OK;
	TP_REQUIRE(ctx, d_pix && d_cad && d_fit && h_index && h_p_offset && h_npix && h_ncad && d_P && d_fit_out, "tp_halo_gather_stack: null pointer");
	std::vector<GatherProb> probs;
	int32_t max_ncad = 0;
	const char* bad = gather_table(g, n_run, h_index, h_p_offset, h_npix, h_ncad, probs, max_ncad);
	TP_REQUIRE(ctx, !bad, bad);
	if (max_ncad == 0) return TP_OK;
	DevBlocks dev(ctx);
	int32_t* dstamps = dev.get<int32_t>((uint64_t)n_targets * 4);
	GatherProb* dprobs = dev.get<GatherProb>(n_run);
	if (dev.rc != TP_OK) return dev.rc;
	rc = upload(ctx, dstamps, h_stamps, (size_t)n_targets * 4);
	if (rc == TP_OK) rc = upload(ctx, dprobs, probs);
	if (rc != TP_OK) return rc;
	TP_LAUNCH(ctx, TPK_HALO_GATHER, tp_halo_gather_kernel, dim3((unsigned)((max_ncad + kGatherRows - 1) / kGatherRows), (unsigned)n_run), dim3(kThreads), 0,
		g, d_images, (const int32_t*)dstamps, (const GatherProb*)dprobs, d_pix, d_cad, d_fit, d_P, d_fit_out);
	TP_LAUNCH_CHECK(ctx, "tp_halo_gather_kernel");
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_halo_outputs_stack(tp_ctx* ctx, const float* d_images_err, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int32_t row0,
	int32_t col0, int32_t n_targets, const int32_t* h_stamps, int32_t height, int32_t width, int32_t n_seg, const int32_t* h_seg,
	const int32_t* d_pix, const int32_t* d_cadpos, int32_t n_run, const int32_t* h_index, const int32_t* h_npix, const int32_t* h_ncad,
	const uint8_t* d_fit, const double* d_w, const double* d_l, const int32_t* d_status, const double* h_normfactor, double* d_median,
	double* d_corr, double* d_flux, double* d_flux_err, double* d_weightmap)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const StackGeom g{n_frames, frame_rows, frame_cols, row0, col0, height, width, n_seg, n_targets};
	int rc = stack_checks(ctx, g, d_images_err, h_stamps, h_seg, true);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, n_run >= 0 && n_run <= 65535, "tp_halo_outputs_stack: 0 .. 65535 problems per call");
	TP_REQUIRE(ctx, d_pix && d_cadpos && h_normfactor && d_median && d_corr && d_flux && d_flux_err && d_weightmap, "tp_halo_outputs_stack: null pointer");
	TP_REQUIRE(ctx, n_run == 0 || (h_index && h_npix && h_ncad && d_fit && d_w && d_l && d_status), "tp_halo_outputs_stack: null pointer");
	// tables, uploads, launches
	std::vector<NormProb> probs;
	std::vector<int32_t> run;
	const char* bad = norm_table(g, n_run, h_index, h_npix, h_ncad, probs, run);
	TP_REQUIRE(ctx, !bad, bad);
	DevBlocks dev(ctx);
	int32_t* dstamps = dev.get<int32_t>((uint64_t)n_targets * 4);
	NormProb* dprobs = dev.get<NormProb>(probs.size());
	int32_t* drun = dev.get<int32_t>(run.size());
	int32_t* dseg = dev.get<int32_t>(n_frames);
	double* dnorm = dev.get<double>(n_targets);
	if (dev.rc != TP_OK) return dev.rc;
	rc = upload(ctx, dstamps, h_stamps, (size_t)n_targets * 4);
	if (rc == TP_OK) rc = upload(ctx, dprobs, probs);
	if (rc == TP_OK) rc = upload(ctx, drun, run);
	if (rc == TP_OK) rc = upload(ctx, dseg, h_seg, (size_t)n_frames);
	if (rc == TP_OK) rc = upload(ctx, dnorm, h_normfactor, (size_t)n_targets);
	if (rc != TP_OK) return rc;
	TP_LAUNCH(ctx, TPK_HALO_NORM, tp_halo_norm_kernel, dim3((unsigned)run.size()), dim3(kThreads), 0, g, (const int32_t*)drun, (const NormProb*)dprobs,
		d_pix, d_fit, d_w, d_l, d_median, d_weightmap);
	TP_LAUNCH_CHECK(ctx, "tp_halo_norm_kernel");
	TP_LAUNCH(ctx, TPK_HALO_LIGHTCURVE, tp_halo_lightcurve_kernel, dim3((unsigned)((n_frames + kThreads / 64 - 1) / (kThreads / 64)), (unsigned)n_targets),
		dim3(kThreads), 0, g, d_images_err, (const int32_t*)dstamps, (const int32_t*)dseg, (const int32_t*)drun, (const NormProb*)dprobs, d_cadpos,
		d_l, d_status, (const double*)d_median, (const double*)d_weightmap, (const double*)dnorm, d_corr, d_flux, d_flux_err);
	TP_LAUNCH_CHECK(ctx, "tp_halo_lightcurve_kernel");
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return TP_OK;
	TP_API_END(ctx)
}
