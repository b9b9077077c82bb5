// linpsf_plan.hip -- the plan of the LinPSF fit (P2..P4) and the coefficients it asks for.
//
// Three kernels ahead of the fit kernels (linpsf.hip: the vector ALUs; linpsf_mfma.hip: the matrix cores):
//   grid  tp_linpsf_grid_kernel: whether the uniform-grid forms apply at all;
//   plan  tp_linpsf_plan_kernel: per target which kernel fits it, the boxes of its stars over all cadences, the segments, union list
//         and tile masks of the matrix-core fit, its place in the coefficient stores and the order of its cadences.  WHAT it decides
//         is stated in linpsf_plan_rules.h (no device code; held to tests/linpsf_common.plan_class on the CPU); the kernel is the
//         parallel plumbing around those rules, in named steps over one PlanShared;
//   coef  tp_linpsf_coef_kernel: the biquartic coefficients of every polynomial item and the A-operand images of the matrix-core
//         segments, contracted from the target's table staged in LDS.
// The polynomial form and what was measured for the three-kernel split are described in linpsf.hip.
#include "linpsf_common.h"
#include <type_traits>

namespace {

using namespace tp_prf;
using namespace tp_linpsf;

// Decides on the device (the knots live there) whether the uniform-grid forms apply: totals[kTotGeneral] = 1 if not.  The plan
// kernel then does nothing and the host, which reads the totals anyway, sends every target to the general kernels.
__global__ __launch_bounds__(64) void tp_linpsf_grid_kernel(const double* __restrict__ tx, const double* __restrict__ ty, int n, double cutoff, int force,
	unsigned long long* __restrict__ totals)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const bool ok = !force && (cutoff <= 5.25) && uniform_grid_ok(tx, n, cutoff) && uniform_grid_ok(ty, n, cutoff);
	if (!ok) totals[kTotGeneral] = 1ull;
}

// What a workgroup of the plan kernel keeps in LDS (one static instance; the cadence keys of the sort are dynamic LDS behind it).
struct PlanShared {
	double spos[4][kMfmaStars][4];      // per wavefront and star: min / max of the row and column position
	double srange[kMfmaStars][4];       // ... over the workgroup
	double kn[160], kny[160];
	SegPlan seg[kMfmaSegs];             // the segments the series is cut into
	StarPlan spl[kMaxStars];
	StarBox sbox[kMaxStars];
	// matrix-core path: the knot intervals every star visits per 16-cadence tile (x lowest / highest, y lowest / highest; the
	// sentinel kTileNone / kTileNoneHigh: no valid position in the tile)
	alignas(8) short tr[kMfmaStars][kMfmaCadTiles][4];
	unsigned pkeys[kMfmaPixels];
	unsigned tiles[kMfmaStars], etiles[kMfmaStars];
	int nseg, walk, fallback, ok, nkeys, path;
};

// what the plan kernel writes
struct PlanOut {
	StarPlan* __restrict__ plans; int32_t* __restrict__ todo; unsigned long long* __restrict__ totals; int32_t* __restrict__ order;
	MPlan* __restrict__ mplans; uint16_t* __restrict__ ulist; uint8_t* __restrict__ usig; int32_t* __restrict__ class_lists;
	SegPlan* __restrict__ segs; int32_t* __restrict__ seg_lists;
};

// step 1: the knots, empty boxes, no tiles, the polynomial path until something better is found
__device__ __forceinline__ void plan_init(const FitArgs& a, PlanShared& sh, int tid)
{
	if (tid == 0) { sh.ok = 0; sh.nkeys = 0; sh.path = kPathPoly; sh.nseg = 0; }
	for (int i = tid; i < a.n + 4; i += 256) { sh.kn[i] = a.knots_x[i]; sh.kny[i] = a.knots_y[i]; }
	if (tid < kMaxStars) box_clear(sh.sbox[tid]);
	if (tid < kMfmaStars) { sh.tiles[tid] = 0u; sh.etiles[tid] = 0u; }
}

// the knot intervals star s visits in the 16-cadence tile of cadence k: consecutive lanes hold consecutive cadences, 16 of them
// are one tile and reduce together
__device__ __forceinline__ void plan_record_tile(PlanShared& sh, int s, int k, int tid, bool in_series, bool valid, int ax0, int by0)
{
	int t0 = valid ? ax0 : kTileNone, t1 = valid ? ax0 : kTileNoneHigh, t2 = valid ? by0 : kTileNone, t3 = valid ? by0 : kTileNoneHigh;
#pragma unroll
	for (int off = 1; off < 16; off <<= 1) {
		const int o0 = __shfl_xor(t0, off, 64), o1 = __shfl_xor(t1, off, 64), o2 = __shfl_xor(t2, off, 64), o3 = __shfl_xor(t3, off, 64);
		t0 = (o0 < t0) ? o0 : t0; t1 = (o1 > t1) ? o1 : t1; t2 = (o2 < t2) ? o2 : t2; t3 = (o3 > t3) ? o3 : t3;
	}
	if ((tid & 15) == 0 && in_series && (k >> 4) < kMfmaCadTiles) {
		const bool any = t1 >= t0;
		sh.tr[s][k >> 4][0] = any ? tile_record(t0) : (short)kTileNone; sh.tr[s][k >> 4][1] = any ? tile_record(t1) : (short)kTileNoneHigh;
		sh.tr[s][k >> 4][2] = any ? tile_record(t2) : (short)kTileNone; sh.tr[s][k >> 4][3] = any ? tile_record(t3) : (short)kTileNoneHigh;
	}
}

// step 2: the series of star s -- its box, its interval ranges per tile of cadences, the rectangle its position sweeps
__device__ __forceinline__ void plan_scan_star(const FitArgs& a, PlanShared& sh, int s, int64_t s0, int tid, bool want, double h, double hy)
{
	int lo[4] = {kBoxNone, kBoxNone, kBoxNone, kBoxNone}, hi[4] = {-kBoxNone, -kBoxNone, -kBoxNone, -kBoxNone};
	double pr[4] = {1e300, -1e300, 1e300, -1e300};   // row min, row max, column min, column max over the valid cadences
	// (whole rounds of 256 cadences, so that the 16 lanes of a tile of cadences reduce together)
	for (int k = tid; k < ((a.n_cad + 255) & ~255); k += 256) {
		const bool in_series = k < a.n_cad;
		const double srow = in_series ? a.pos_row[(s0 + s) * a.pos_pitch + k] : __builtin_nan(""), scol = in_series ? a.pos_col[(s0 + s) * a.pos_pitch + k] : __builtin_nan("");
		double phx, phy; int ax0, by0;
		const bool vx = axis_phase(sh.kn, a.n, scol, h, phx, ax0);
		const bool vy = axis_phase(sh.kny, a.n, srow, hy, phy, by0);
		if (want && s < kMfmaStars) plan_record_tile(sh, s, k, tid, in_series, vx && vy, ax0, by0);
		if (vx && vy) {
			int v0[4], v1[4];
			cadence_box(ax0, by0, srow, scol, a.cutoff, v0, v1);
#pragma unroll
			for (int e = 0; e < 4; ++e) { lo[e] = (v0[e] < lo[e]) ? v0[e] : lo[e]; hi[e] = (v1[e] > hi[e]) ? v1[e] : hi[e]; }
			pr[0] = fmin(pr[0], srow); pr[1] = fmax(pr[1], srow); pr[2] = fmin(pr[2], scol); pr[3] = fmax(pr[3], scol);
		}
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const int l2 = __shfl_xor(lo[e], off, 64), h2 = __shfl_xor(hi[e], off, 64);
			lo[e] = (l2 < lo[e]) ? l2 : lo[e];
			hi[e] = (h2 > hi[e]) ? h2 : hi[e];
		}
		pr[0] = fmin(pr[0], __shfl_xor(pr[0], off, 64)); pr[1] = fmax(pr[1], __shfl_xor(pr[1], off, 64));
		pr[2] = fmin(pr[2], __shfl_xor(pr[2], off, 64)); pr[3] = fmax(pr[3], __shfl_xor(pr[3], off, 64));
	}
	if ((tid & 63) == 0) {
		if (hi[0] >= lo[0]) {
			atomicMin(&sh.sbox[s].axmin, lo[0]); atomicMax(&sh.sbox[s].axmax, hi[0]);
			atomicMin(&sh.sbox[s].bymin, lo[1]); atomicMax(&sh.sbox[s].bymax, hi[1]);
			atomicMin(&sh.sbox[s].jmin, lo[2]); atomicMax(&sh.sbox[s].jmax, hi[2]);
			atomicMin(&sh.sbox[s].imin, lo[3]); atomicMax(&sh.sbox[s].imax, hi[3]);
		}
		if (s < kMfmaStars) {
#pragma unroll
			for (int e = 0; e < 4; ++e) sh.spos[tid >> 6][s][e] = pr[e];
		}
	}
}

// step 3 (one thread): the boxes closed into the stars' plans and position ranges, the vector-ALU kernel the target falls back to,
// and -- the matrix-core path: the series cut into segments of 16-cadence tiles inside which no star visits more than kMfmaSpan
// knot intervals per axis -- either the common case, the whole series as one segment, or a request for the walk of the tiles
__device__ __forceinline__ void plan_close_boxes(const FitArgs& a, PlanShared& sh, int target, int ns, bool want)
{
	for (int s = 0; s < ns; ++s) star_plan_of(sh.sbox[s], a.height, a.width, sh.spl[s]);
	sh.fallback = fallback_path(sh.spl, ns);
	for (int s = 0; s < ns && s < kMfmaStars; ++s) {
		sh.srange[s][0] = fmin(fmin(sh.spos[0][s][0], sh.spos[1][s][0]), fmin(sh.spos[2][s][0], sh.spos[3][s][0]));
		sh.srange[s][1] = fmax(fmax(sh.spos[0][s][1], sh.spos[1][s][1]), fmax(sh.spos[2][s][1], sh.spos[3][s][1]));
		sh.srange[s][2] = fmin(fmin(sh.spos[0][s][2], sh.spos[1][s][2]), fmin(sh.spos[2][s][2], sh.spos[3][s][2]));
		sh.srange[s][3] = fmax(fmax(sh.spos[0][s][3], sh.spos[1][s][3]), fmax(sh.spos[2][s][3], sh.spos[3][s][3]));
	}
	int nseg = 0;
	sh.walk = 0;
	if (segments_possible(want, a.height, a.width, a.n_cad)) {
		int lo[kMfmaStars][2], hi[kMfmaStars][2];
		if (whole_series_ranges(sh.sbox, ns, lo, hi)) { emit_segment(sh.seg[0], target, 0, (a.n_cad + 15) >> 4, lo, hi, ns, sh.spl); nseg = 1; }
		else sh.walk = 1;   // the first wavefront walks the tiles (plan_walk_tiles)
	}
	sh.nseg = nseg;
}

// a window of 64 tiles: lane j holds the knot intervals of tile pos + j, an inclusive min / max scan gives every lane the range
// pl .. pu of [segment start, its tile] (clo / chi: the open segment's range before the window); false where that goes beyond the span.
// (__shfl_up hands a lane below `off` its own value back, and a minimum / maximum with itself changes nothing: the steps of the scan
// need no test of the lane -- with one, its six masks stay in scalar registers all through the walk, eight more than there are)
__device__ __forceinline__ bool plan_scan_window(const PlanShared& sh, int ns, int lane, int t, bool valid, const int (&clo)[kMfmaStars][2], const int (&chi)[kMfmaStars][2],
	int (&pl)[kMfmaStars][2], int (&pu)[kMfmaStars][2])
{
	bool fits = true;
#pragma unroll
	for (int s = 0; s < kMfmaStars; ++s) {
#pragma unroll
		for (int e = 0; e < 2; ++e) {
			int l = (valid && s < ns) ? (int)sh.tr[s][valid ? t : 0][2 * e] : kTileNone, u = (valid && s < ns) ? (int)sh.tr[s][valid ? t : 0][2 * e + 1] : kTileNoneHigh;
			if (lane == 0) { l = (clo[s][e] < l) ? clo[s][e] : l; u = (chi[s][e] > u) ? chi[s][e] : u; }
#pragma unroll
			for (int off = 1; off < 64; off <<= 1) {
				const int ol = __shfl_up(l, off, 64), ou = __shfl_up(u, off, 64);
				l = (ol < l) ? ol : l; u = (ou > u) ? ou : u;
			}
			pl[s][e] = l; pu[s][e] = u;
			if (!span_fits(l, u)) fits = false;
		}
	}
	return fits;
}

// step 4 (the first wavefront): greedy segmentation, a window of 64 tiles at a time: the first lane whose range goes beyond the
// span ends the segment before its tile.  (One thread walking the tiles through LDS took 40 us per target.)  A star that goes beyond
// the span inside ONE tile (jitter of a third of a pixel within 16 cadences) or more than kMfmaSegs segments leave no segments:
// the vector-ALU kernels take the target.
__device__ __forceinline__ void plan_walk_tiles(const FitArgs& a, PlanShared& sh, int target, int ns, int lane)
{
	const int ntile = (a.n_cad + 15) >> 4;
	int nseg = 0, seg_start = 0, pos = 0;
	bool ok = true;
	int clo[kMfmaStars][2], chi[kMfmaStars][2];   // the range of the open segment up to the window (wave-uniform)
	ranges_clear(clo, chi);
	while (pos < ntile && ok) {
		const int t = pos + lane;
		const bool valid = t < ntile;
		int pl[kMfmaStars][2], pu[kMfmaStars][2];
		const bool fits = plan_scan_window(sh, ns, lane, t, valid, clo, chi, pl, pu);
		const unsigned long long bad = __ballot(valid && !fits);
		if (bad == 0ull) {
			const int lastl = (ntile - 1 - pos < 63) ? (ntile - 1 - pos) : 63;
#pragma unroll
			for (int s = 0; s < kMfmaStars; ++s)
#pragma unroll
				for (int e = 0; e < 2; ++e) { clo[s][e] = __shfl(pl[s][e], lastl, 64); chi[s][e] = __shfl(pu[s][e], lastl, 64); }
			pos += 64;
			continue;
		}
		const int c = __builtin_ctzll(bad);
		if (c == 0 && pos == seg_start) { ok = false; break; }   // one tile of cadences alone goes beyond the span
		int lo[kMfmaStars][2], hi[kMfmaStars][2];
#pragma unroll
		for (int s = 0; s < kMfmaStars; ++s)
#pragma unroll
			for (int e = 0; e < 2; ++e) {
				const int sl = __shfl(pl[s][e], (c > 0) ? (c - 1) : 0, 64), su = __shfl(pu[s][e], (c > 0) ? (c - 1) : 0, 64);
				lo[s][e] = (c > 0) ? sl : clo[s][e]; hi[s][e] = (c > 0) ? su : chi[s][e];
				clo[s][e] = kTileNone; chi[s][e] = kTileNoneHigh;
			}
		if (nseg >= kMfmaSegs) { ok = false; break; }
		if (lane == 0) emit_segment(sh.seg[nseg], target, seg_start, pos + c, lo, hi, ns, sh.spl);
		++nseg;
		seg_start = pos = pos + c;
	}
	if (ok) {
		if (nseg >= kMfmaSegs) ok = false;
		else { if (lane == 0) emit_segment(sh.seg[nseg], target, seg_start, ntile, clo, chi, ns, sh.spl); ++nseg; }
	}
	if (lane == 0) sh.nseg = ok ? nseg : 0;
}

// step 5: the union list -- the pixels some star can reach at some cadence, ordered by their keys -- and the tiles of 16 list
// entries every star touches; a large stamp (more than kMfmaPixels of them) leaves the target to the vector-ALU kernels
__device__ __forceinline__ void plan_union_list(const FitArgs& a, PlanShared& sh, const PlanOut& o, int target, int ns, int tid)
{
	const int npix = a.height * a.width;
	const double reach = pixel_reach2(a.cutoff), always = pixel_always2(a.cutoff);
	for (int p = tid; p < npix; p += 256) {
		const int i = p / a.width, j = p - i * a.width;
		unsigned sig = 0u, edge = 0u;
		for (int s = 0; s < ns; ++s) {
			if (sh.spl[s].nc <= 0) continue;
			const unsigned m = pixel_membership(i, j, sh.srange[s], reach, always);
			sig |= (m & 1u) << s; edge |= (m >> 1) << s;
		}
		if (sig) {
			const int idx = atomicAdd(&sh.nkeys, 1);
			if (idx < kMfmaPixels) sh.pkeys[idx] = pixel_key(sig, edge, p);
		}
	}
	__syncthreads();
	const int nk = sh.nkeys;
	if (nk > kMfmaPixels) { if (tid == 0) sh.path = sh.fallback; }
	else {
		uint16_t* ul = o.ulist + (int64_t)target * kMfmaPixels;
		uint8_t* us = o.usig + (int64_t)target * kMfmaPixels;
		if (tid < nk) {
			const unsigned key = sh.pkeys[tid];
			int r = 0;
			for (int q = 0; q < nk; ++q) r += (sh.pkeys[q] < key) ? 1 : 0;
			ul[r] = key_pixel(key);
			us[r] = key_usig(key);
			for (int s = 0; s < ns; ++s) {
				if (key_sig(key) & (1u << s)) atomicOr(&sh.tiles[s], 1u << (r >> 4));
				if (key_edge(key) & (1u << s)) atomicOr(&sh.etiles[s], 1u << (r >> 4));
			}
		} else if (tid < kMfmaPixels) { ul[tid] = (uint16_t)0xffffu; us[tid] = (uint8_t)0; }
	}
	__syncthreads();
}

// step 6a (one thread): a target of the matrix cores -- its segments' images within the LDS of its class -- takes its place in the
// matrix-core store and in the lists of its class (one launch per star count); false: the vector-ALU kernels take it
__device__ __forceinline__ bool plan_commit_mfma(PlanShared& sh, const PlanOut& o, int target, int ns, int n_targets)
{
	MPlan mp;
	make_mplan(mp, sh.nkeys, sh.nseg, ns, sh.tiles, sh.etiles);
	long long total;
	if (!size_segments(sh.seg, sh.nseg, ns, mp, total)) return false;
	const long long base = (long long)atomicAdd(&o.totals[kTotKDoubles], (unsigned long long)total);
	o.mplans[target] = mp;
	const int cls = ns - 1;
	const unsigned long long sat = atomicAdd(&o.totals[kTotSeg0 + cls], (unsigned long long)sh.nseg);
	for (int i = 0; i < sh.nseg; ++i) {
		sh.seg[i].koff += base;
		o.segs[(int64_t)target * kMfmaSegs + i] = sh.seg[i];
		o.seg_lists[(int64_t)cls * n_targets * kMfmaSegs + (int64_t)sat + i] = target * kMfmaSegs + i;
	}
	for (int s = 0; s < ns; ++s) o.plans[(int64_t)target * kMaxStars + s] = sh.spl[s];
	o.todo[target] = kPathMfma;
	const unsigned long long at = atomicAdd(&o.totals[kTotClass0 + cls], 1ull);
	o.class_lists[(int64_t)cls * n_targets + (int64_t)at] = target;
	return true;
}

// step 6 (one thread): the target's path is final; its share of the stores (one atomic per target) and what the kernels after this
// one read.  Sets sh.ok for the targets of the polynomial fit: they need the order of their cadences.
__device__ __forceinline__ void plan_commit(PlanShared& sh, const PlanOut& o, int target, int ns, int n_targets)
{
	int path = sh.path;
	if (path == kPathMfma && !plan_commit_mfma(sh, o, target, ns, n_targets)) path = sh.fallback;
	if (path == kPathDirect) { o.todo[target] = kPathDirect; atomicAdd(&o.totals[kTotDirectTargets], 1ull); }
	else if (path == kPathPoly) {
		const long long items = poly_item_offsets(sh.spl, ns);
		const long long base = (long long)atomicAdd(&o.totals[kTotPolyItems], (unsigned long long)items);
		atomicAdd(&o.totals[kTotPolyTargets], 1ull);
		for (int s = 0; s < ns; ++s) { sh.spl[s].item_off += base; o.plans[(int64_t)target * kMaxStars + s] = sh.spl[s]; }
		sh.ok = 1;
	}
}

// step 7: the order in which the fit kernel walks the cadences: sorted by the origins of all stars, so that the 64 cadences of a
// wavefront share their polynomial coefficients (the jitter straddles a knot boundary in most targets)
__device__ __forceinline__ void plan_cadence_order(const FitArgs& a, const PlanShared& sh, unsigned long long* skeys, int32_t* ord, int sort_n, int64_t s0, int ns, int tid,
	double h, double hy)
{
	if (sort_n <= 0) { for (int k = tid; k < a.n_cad; k += 256) ord[k] = k; return; }
	for (int k = tid; k < sort_n; k += 256) {
		unsigned long long key = ~0ull;
		if (k < a.n_cad) {
			key = 0;
			for (int s = 0; s < ns; ++s) {
				double phx, phy; int ax0, by0;
				const bool vx = axis_phase(sh.kn, a.n, a.pos_col[(s0 + s) * a.pos_pitch + k], h, phx, ax0);
				const bool vy = axis_phase(sh.kny, a.n, a.pos_row[(s0 + s) * a.pos_pitch + k], hy, phy, by0);
				key = cadence_key_star(key, sh.spl[s], vx && vy, ax0, by0);
			}
			key = cadence_key_close(key, k);
		}
		skeys[k] = key;
	}
	__syncthreads();
	for (int size = 2; size <= sort_n; size <<= 1) {
		for (int stride = size >> 1; stride > 0; stride >>= 1) {
			for (int t = tid; t < sort_n / 2; t += 256) {
				const int lo = ((t / stride) * (stride << 1)) + (t % stride), hi = lo + stride;
				const bool up = ((lo & size) == 0);
				const unsigned long long x = skeys[lo], y = skeys[hi];
				if ((x > y) == up) { skeys[lo] = y; skeys[hi] = x; }
			}
			__syncthreads();
		}
	}
	for (int k = tid; k < a.n_cad; k += 256) ord[k] = key_cadence(skeys[k]);
}

// totals: kTotPolyItems items (25 doubles each) of the polynomial store; kTotKDoubles doubles of the matrix-core store (laid behind
// it); kTotPolyTargets targets left to the vector-ALU fit; kTotClass0 + c targets of class c of the matrix-core fit (class_lists[c][..])
__global__ __launch_bounds__(256) void tp_linpsf_plan_kernel(FitArgs a, PlanOut o, int sort_n, int use_mfma, int n_targets)
{
	extern __shared__ unsigned long long skeys[];   // [sort_n] (key of the cadence's origins) * 8192 + cadence, or nothing
	__shared__ PlanShared sh;
	const int target = blockIdx.x, tid = threadIdx.x;
	const int64_t s0 = a.star_offsets[target];
	const int ns = (int)(a.star_offsets[target + 1] - s0);
	if (o.totals[kTotGeneral] != 0) return;   // tp_linpsf_grid_kernel found a grid / cut-off the uniform forms cannot take: the general kernels fit every target
	if (ns > kMaxStars) return;   // the many-star kernel's targets
	const bool want = want_segments(use_mfma, ns);
	plan_init(a, sh, tid);
	__syncthreads();
	const double h = sh.kn[5] - sh.kn[4], hy = sh.kny[5] - sh.kny[4];
	for (int s = 0; s < ns; ++s) plan_scan_star(a, sh, s, s0, tid, want, h, hy);
	__syncthreads();
	if (tid == 0) plan_close_boxes(a, sh, target, ns, want);
	__syncthreads();
	if (sh.walk && tid < 64) plan_walk_tiles(a, sh, target, ns, tid);
	__syncthreads();
	if (tid == 0) sh.path = (sh.nseg > 0) ? kPathMfma : sh.fallback;
	__syncthreads();
	if (sh.path == kPathMfma) plan_union_list(a, sh, o, target, ns, tid);
	if (tid == 0) plan_commit(sh, o, target, ns, n_targets);
	__syncthreads();
	if (!sh.ok) return;
	plan_cadence_order(a, sh, skeys, o.order + (int64_t)target * a.n_cad, sort_n, s0, ns, tid, h, hy);
}

// the 25 coefficients (times h2) of the 13 x 13 table patch at (ax, by): kk[e][b], e = power of phi_x, b = power of phi_y
__device__ __forceinline__ void patch_coefficients(const double* __restrict__ C, int n, int ax, int by, double h2, double (&kk)[5][5])
{
#pragma unroll
	for (int e = 0; e < 5; ++e)
#pragma unroll
		for (int bcol = 0; bcol < 5; ++bcol) kk[e][bcol] = 0.0;
	const double* c0 = C + (int64_t)ax * n + by;
#pragma unroll 1
	for (int pp = 0; pp < 13; ++pp) {
		const double* r = c0 + pp * n;
		double rv[13];
#pragma unroll
		for (int q = 0; q < 13; ++q) rv[q] = r[q];
		const double e0 = kEdgePoly[pp][0], e1 = kEdgePoly[pp][1], e2 = kEdgePoly[pp][2], e3 = kEdgePoly[pp][3], e4 = kEdgePoly[pp][4];
#pragma unroll
		for (int bcol = 0; bcol < 5; ++bcol) {
			double t = 0.0;
#pragma unroll
			for (int q = 0; q < 13; ++q) t = __builtin_fma(kEdgePoly[q][bcol], rv[q], t);
			kk[0][bcol] = __builtin_fma(e0, t, kk[0][bcol]);
			kk[1][bcol] = __builtin_fma(e1, t, kk[1][bcol]);
			kk[2][bcol] = __builtin_fma(e2, t, kk[2][bcol]);
			kk[3][bcol] = __builtin_fma(e3, t, kk[3][bcol]);
			kk[4][bcol] = __builtin_fma(e4, t, kk[4][bcol]);
		}
	}
#pragma unroll
	for (int e = 0; e < 5; ++e)
#pragma unroll
		for (int bcol = 0; bcol < 5; ++bcol) kk[e][bcol] *= h2;
}

// The same contraction for the `na` consecutive intervals (ax, by), (ax + 1, by) .. along x at once: their 13 x 13 patches are
// 13 + na - 1 table rows, and the inner sums t = sum_q E[q][b] C[row][by + q] of a row serve every interval that holds the row
// (2 340 -> 1 560 multiply-adds for two intervals, 3 510 -> 2 100 for three).  Every kk[ca] gets exactly the operations
// patch_coefficients gives it, in the same order: bit-identical.  Rows ax .. ax + 12 + na - 1 must lie inside the table.
__device__ __forceinline__ void patch_coefficients_along_x(const double* __restrict__ C, int n, int ax, int by, double h2, int na, double (&kk)[3][5][5])
{
#pragma unroll
	for (int ca = 0; ca < 3; ++ca)
#pragma unroll
		for (int e = 0; e < 5; ++e)
#pragma unroll
			for (int bcol = 0; bcol < 5; ++bcol) kk[ca][e][bcol] = 0.0;
	const double* c0 = C + (int64_t)ax * n + by;
#pragma unroll 1
	for (int row = 0; row < 12 + na; ++row) {
		const double* r = c0 + row * n;
		double rv[13], t[5];
#pragma unroll
		for (int q = 0; q < 13; ++q) rv[q] = r[q];
#pragma unroll
		for (int bcol = 0; bcol < 5; ++bcol) {
			double v = 0.0;
#pragma unroll
			for (int q = 0; q < 13; ++q) v = __builtin_fma(kEdgePoly[q][bcol], rv[q], v);
			t[bcol] = v;
		}
#pragma unroll
		for (int ca = 0; ca < 3; ++ca) {
			const int pp = row - ca;
			if (ca < na && pp >= 0 && pp < 13) {   // uniform
				const double e0 = kEdgePoly[pp][0], e1 = kEdgePoly[pp][1], e2 = kEdgePoly[pp][2], e3 = kEdgePoly[pp][3], e4 = kEdgePoly[pp][4];
#pragma unroll
				for (int bcol = 0; bcol < 5; ++bcol) {
					kk[ca][0][bcol] = __builtin_fma(e0, t[bcol], kk[ca][0][bcol]);
					kk[ca][1][bcol] = __builtin_fma(e1, t[bcol], kk[ca][1][bcol]);
					kk[ca][2][bcol] = __builtin_fma(e2, t[bcol], kk[ca][2][bcol]);
					kk[ca][3][bcol] = __builtin_fma(e3, t[bcol], kk[ca][3][bcol]);
					kk[ca][4][bcol] = __builtin_fma(e4, t[bcol], kk[ca][4][bcol]);
				}
			}
		}
	}
#pragma unroll
	for (int ca = 0; ca < 3; ++ca)
#pragma unroll
		for (int e = 0; e < 5; ++e)
#pragma unroll
			for (int bcol = 0; bcol < 5; ++bcol) kk[ca][e][bcol] *= h2;
}

constexpr int kCoefThreads = 512;

// the matrix-core images of a target (table C staged in LDS)
__device__ __forceinline__ void coef_mfma_images(const FitArgs& a, const double* C, int n, double h2, int target, int tid, int ns,
	const MPlan* __restrict__ mplans, const uint16_t* __restrict__ ulist, const uint8_t* __restrict__ usig, double* __restrict__ kstore, const SegPlan* __restrict__ segs)
{
	// matrix-core layout (linpsf_mfma.hip): per (star, tile of the star) the A operands of the MFMA steps, lane = (group g,
	// pixel u of the tile).  The coefficients are those of the tensor-product quartic spline over the na x nb knot intervals
	// the star visits, in the basis {1, X, X^2, X^3, X^4, (X-1)+^4, (X-2)+^4} x {the same in Y}: ce[e][d] (e, d <= 4) is the
	// biquartic of interval (0, 0); a quartic spline changes only its leading coefficient at a knot, so the coefficient of
	// (X-a)+^4 Y^d is K(a,0)[4][d] - K(a-1,0)[4][d], of X^e (Y-b)+^4 it is K(0,b)[e][4] - K(0,b-1)[e][4], and of (X-a)+^4 (Y-b)+^4
	// the second difference of K[4][4] -- every interval's 13 x 13 patch is contracted as for the vector-ALU path.
	// Pixels of the tile the star never reaches get zeros.
	const MPlan mp = mplans[target];
	const uint16_t* ul = ulist + (int64_t)target * kMfmaPixels;
	const uint8_t* us = usig + (int64_t)target * kMfmaPixels;
	// One thread per (pixel of a tile, knot interval): the 13 x 13 patch of that interval is contracted into its 25
	// coefficients; the interval (0, 0) writes the steps that hold C[e][d], e <= 4, d < 4, at once, every interval leaves its
	// K[4][0..4] and K[0..3][4] in LDS, and one thread per pixel then forms the differences and writes the remaining steps.
	// Jobs: one per (segment, star that is on the stamp in it).  A LANE takes one pixel of the star's tiles and one interval
	// along y, and all na intervals along x (patch_coefficients_along_x); the nb lanes of a pixel are neighbours, so the
	// differences across y come from the lane below by one shuffle and those across x are the lane's own -- nothing goes
	// through LDS, and after the table is staged no wavefront waits for another: each takes every (waves)-th unit of 64 / nb
	// pixels of the job list.  (One thread per (pixel, interval) with the differences formed through LDS between two barriers
	// per round of 512 threads, a round per star and segment: 1.09 ms per 10 000 targets, 4.4 ms on the drift scene.)
	struct Job { int na, nb, nt, axmin, bymin, s; unsigned tiles; long long dst; };
	__shared__ Job s_job[kMfmaSegs * kMfmaStars];
	__shared__ int s_njobs;
	if (tid == 0) {
		int nj = 0;
		for (int sgi = 0; sgi < mp.n_seg; ++sgi) {
			const SegPlan sg = segs[(int64_t)target * kMfmaSegs + sgi];
			for (int s = 0; s < ns; ++s) {
				if (sg.na[s] == 0) continue;
				Job j;
				j.na = sg.na[s]; j.nb = sg.nb[s]; j.nt = __popc(mp.tiles[s]); j.axmin = sg.axmin[s]; j.bymin = sg.bymin[s]; j.s = s;
				j.tiles = mp.tiles[s]; j.dst = sg.koff + (long long)sg.ksub[s] * 64;
				s_job[nj++] = j;
			}
		}
		s_njobs = nj;
	}
	__syncthreads();
	const int njobs = s_njobs;
	const int lane = tid & 63, wave = tid >> 6, nwaves = (int)blockDim.x >> 6;
	int unit = 0;                              // units of the job list passed so far (uniform)
	for (int jb = 0; jb < njobs; ++jb) {
		const Job jq = s_job[jb];
		const int na = jq.na, nb = jq.nb, nk = mfma_steps(na, nb);
		const int per = 64 / nb, nitems = jq.nt * 16;
		const int nunits = (nitems + per - 1) / per;
		for (int c = 0; c < nunits; ++c, ++unit) {
			if (unit % nwaves != wave) continue;
			const int li = lane / nb, cb = lane - li * nb;
			const int item = c * per + li;
			const bool mine = li < per && item < nitems;
			double kk[3][5][5];
			int r = 0, u = 0;
			bool reach = false;
			int ax = 0, by = 0;
			if (mine) {
				r = item >> 4; u = item & 15;
				unsigned m = jq.tiles;
				for (int q = 0; q < r; ++q) m &= m - 1;          // drop the r lowest set bits
				const int slot = (__ffs(m) - 1) * 16 + u;
				const unsigned pix = ul[slot];
				if (pix != 0xffffu && ((us[slot] >> jq.s) & 1)) {
					const int i = (int)pix / a.width, j = (int)pix - i * a.width;
					ax = jq.axmin + 9 * j; by = (jq.bymin + cb) + 9 * i;
					by = by < 0 ? 0 : (by > n - 13 ? n - 13 : by);
					reach = true;
				}
			}
			if (reach && ax >= 0 && ax + na - 1 <= n - 13) {
				patch_coefficients_along_x(C, n, ax, by, h2, na, kk);
			} else {
#pragma unroll
				for (int ca = 0; ca < 3; ++ca) {
					if (reach && ca < na) {                  // an interval beyond the table's edge: clamped one by one
						int axc = ax + ca;
						axc = axc < 0 ? 0 : (axc > n - 13 ? n - 13 : axc);
						patch_coefficients(C, n, axc, by, h2, kk[ca]);
					} else {
#pragma unroll
						for (int e = 0; e < 5; ++e)
#pragma unroll
							for (int d = 0; d < 5; ++d) kk[ca][e][d] = 0.0;
					}
				}
			}
			// what the lane below (same pixel, interval cb - 1) holds of K[0][0..3][4] and K[ca][4][4]; zero below interval 0
			double lo_e4[4], lo_44[3];
#pragma unroll
			for (int e = 0; e < 4; ++e) { const double v = __shfl_up(kk[0][e][4], 1, 64); lo_e4[e] = (cb > 0) ? v : 0.0; }
#pragma unroll
			for (int ca = 0; ca < 3; ++ca) { const double v = __shfl_up(kk[ca][4][4], 1, 64); lo_44[ca] = (cb > 0) ? v : 0.0; }
			if (!mine) continue;
			double* dst = kstore + jq.dst + (int64_t)r * nk * 64 + u;
			// ce[4 + a][d] (d < 4), ce[e][4 + b] (e < 4), ce[4 + a][4 + b]: first differences along the axis that leaves interval 0,
			// the second difference of K[4][4] off both axes (operations and their order as in the LDS version)
			auto corner = [&](int ca) -> double {
				const double here = kk[ca][4][4], left = (ca > 0) ? kk[ca > 0 ? ca - 1 : 0][4][4] : 0.0;
				const double below = lo_44[ca], diag = (ca > 0) ? lo_44[ca > 0 ? ca - 1 : 0] : 0.0;
				return ((here - left) - below) + diag;
			};
			if (cb == 0) {
#pragma unroll
				for (int e = 0; e < 5; ++e)
#pragma unroll
					for (int g = 0; g < 4; ++g) dst[e * 64 + g * 16] = kk[0][e][g];
			}
			if (mfma_is22(na, nb)) {
				// 9 steps: y basis 4 with x basis 0..3; {x basis 4, 5 with y basis 4, x basis 0, 1 with y basis 5}; x basis 5 with y
				// basis 0..3; x basis 2..5 with y basis 5
				if (cb == 0) {
#pragma unroll
					for (int g = 0; g < 4; ++g) {
						dst[5 * 64 + g * 16] = kk[0][g][4] - 0.0;
						dst[7 * 64 + g * 16] = kk[1][4][g] - kk[0][4][g];
					}
					dst[6 * 64 + 0 * 16] = corner(0);
					dst[6 * 64 + 1 * 16] = corner(1);
				} else {
					dst[6 * 64 + 2 * 16] = kk[0][0][4] - lo_e4[0];
					dst[6 * 64 + 3 * 16] = kk[0][1][4] - lo_e4[1];
					dst[8 * 64 + 0 * 16] = kk[0][2][4] - lo_e4[2];
					dst[8 * 64 + 1 * 16] = kk[0][3][4] - lo_e4[3];
					dst[8 * 64 + 2 * 16] = corner(0);
					dst[8 * 64 + 3 * 16] = corner(1);
				}
			} else {
				// steps: 5, 6 for y interval 0; 7 .. for the x basis functions 5, 6; then two per further y interval
				const int ystep = 5 + 2 * cb + ((cb >= 1) ? (na - 1) : 0);
#pragma unroll
				for (int g = 0; g < 4; ++g) {
					dst[ystep * 64 + g * 16] = kk[0][g][4] - lo_e4[g];
					double cv = 0.0;
					if (g == 0) cv = corner(0);
					else if (g == 1 && na > 1) cv = corner(1);
					else if (g == 2 && na > 2) cv = corner(2);
					dst[(ystep + 1) * 64 + g * 16] = cv;
				}
				if (cb == 0) {
#pragma unroll
					for (int ca = 1; ca < 3; ++ca) {
						if (ca < na) {
#pragma unroll
							for (int g = 0; g < 4; ++g) dst[(6 + ca) * 64 + g * 16] = kk[ca][4][g] - kk[ca - 1][4][g];
						}
					}
				}
			}
		}
	}
}

// the polynomial items of a target (table C staged in LDS)
__device__ __forceinline__ void coef_poly_items(const double* C, int n, double h2, int target, int tid, int ns, const StarPlan* __restrict__ plans, double* __restrict__ store)
{
	for (int s = 0; s < ns; ++s) {
		const StarPlan p = plans[(int64_t)target * kMaxStars + s];
		const int ncols = p.jmax - p.jmin + 1, nrows = p.imax - p.imin + 1;
		if (p.nc <= 0 || ncols <= 0 || nrows <= 0) continue;
		const int nitems = p.nc * ncols * nrows;
		// one thread per item: the 13 x 13 patch of the table is read once and contracted into all 25 coefficients (the sums
		// run over q inside, over p outside)
		for (int item = tid; item < nitems; item += kCoefThreads) {
			const int pix = item / p.nc, co = item - pix * p.nc;
			const int ii = pix / ncols, jj = pix - ii * ncols;
			const int cx = co / p.nby, cy = co - cx * p.nby;
			int ax = (p.axmin + cx) + 9 * (p.jmin + jj), by = (p.bymin + cy) + 9 * (p.imin + ii);
			ax = ax < 0 ? 0 : (ax > n - 13 ? n - 13 : ax);
			by = by < 0 ? 0 : (by > n - 13 ? n - 13 : by);
			double kk[5][5];
			patch_coefficients(C, n, ax, by, h2, kk);
			double* dst = store + (p.item_off + item) * 25;
#pragma unroll
			for (int e = 0; e < 5; ++e)
#pragma unroll
				for (int bcol = 0; bcol < 5; ++bcol) dst[e * 5 + bcol] = kk[e][bcol];
		}
	}
}

__global__ __launch_bounds__(kCoefThreads) void tp_linpsf_coef_kernel(FitArgs a, const StarPlan* __restrict__ plans, const int32_t* __restrict__ todo,
	double* __restrict__ store, const MPlan* __restrict__ mplans, const uint16_t* __restrict__ ulist, const uint8_t* __restrict__ usig,
	double* __restrict__ kstore, const SegPlan* __restrict__ segs)
{
	extern __shared__ __align__(16) double ctab[];   // the target's coefficient table [n*n]: every patch is read ~5 times over
	const int target = blockIdx.x, tid = threadIdx.x;
	const int path = todo[target];
	if (path == kPathDirect) return;
	const int ns = (int)(a.star_offsets[target + 1] - a.star_offsets[target]);
	if (ns > kMaxStars) return;
	const int n = a.n;
	const double h2 = (a.knots_x[5] - a.knots_x[4]) * (a.knots_y[5] - a.knots_y[4]);
	{
		// the whole table in flight at once (up to 39 doubles per thread for the largest table admitted), then into LDS: one round
		// trip to memory instead of one per slice.  (A workgroup per CU that walks the targets with the next table on its way in
		// registers while this one's patches are contracted: 0.85 against 0.76 ms -- 78 more registers, and the targets' work differs.)
		const double* cg = a.coef + (int64_t)target * n * n;
		constexpr int kPer = (140 * 140 + kCoefThreads - 1) / kCoefThreads;
		double tmp[kPer];
#pragma unroll
		for (int u = 0; u < kPer; ++u) { const int i = u * kCoefThreads + tid; tmp[u] = (i < n * n) ? cg[i] : 0.0; }
#pragma unroll
		for (int u = 0; u < kPer; ++u) { const int i = u * kCoefThreads + tid; if (i < n * n) ctab[i] = tmp[u]; }
	}
	__syncthreads();
	const double* C = ctab;
	if (path == kPathMfma) coef_mfma_images(a, C, n, h2, target, tid, ns, mplans, ulist, usig, kstore, segs);
	else coef_poly_items(C, n, h2, target, tid, ns, plans, store);
}

} // namespace

namespace tp_linpsf {

constexpr size_t kTotalWords = 32;
static_assert(kTotCount <= kTotalWords, "the counters fit their block");

void carve_plan_scratch(uintptr_t base, size_t n_targets, size_t n_cad, bool with_alast, PlanScratch& h)
{
	size_t off = 0;
	auto take = [&](auto*& p, size_t count) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off); off += align256(count * sizeof(*p)); };
	take(h.todo, n_targets); h.todo_bytes = off;
	take(h.plans, n_targets * kMaxStars);
	take(h.total, kTotalWords);
	take(h.order, n_targets * n_cad);
	take(h.mplans, n_targets);
	take(h.ulist, n_targets * kMfmaPixels);
	take(h.usig, n_targets * kMfmaPixels);
	take(h.lists, n_targets * kMfmaClasses);
	take(h.segs, n_targets * kMfmaSegs);
	take(h.seglists, n_targets * kMfmaSegs * kMfmaClasses);
	take(h.alast, with_alast ? n_targets * kMfmaStars * kMfmaPixels : 0);
	h.bytes = off;
}

int run_plan(tp_ctx* ctx, const FitArgs& a, int n_targets, const PlanScratch& h, int use_mfma, unsigned long long (&totals)[kTotCount])
{
	// cadences sorted by origin in LDS (8 bytes per slot, next power of two); beyond 8192 cadences the order stays natural
	int sort_n = 64;
	while (sort_n < a.n_cad) sort_n <<= 1;
	if (sort_n > 8192) sort_n = 0;
	TP_HIP(ctx, hipMemsetAsync(h.todo, 0, h.todo_bytes, ctx->stream));
	TP_HIP(ctx, hipMemsetAsync(h.total, 0, kTotalWords * sizeof(unsigned long long), ctx->stream));
	// The uniform-grid kernels (all but the any-grid ones) need the SPOC layout of the PRF grid: 9 samples per pixel, the table
	// resident in LDS, the cut-off inside the evenly spaced part of the knots.  Whether that holds is decided where the knots are.
	// (a table with axes of different lengths is never the SPOC layout: the general kernels, the only ones that read a.ny)
	const int force = (a.n != a.ny || a.n < 32 || a.n > 140 || !(a.cutoff <= 5.25)) ? 1 : 0;
	hipLaunchKernelGGL(tp_linpsf_grid_kernel, dim3(1), dim3(64), 0, ctx->stream, a.knots_x, a.knots_y, a.n, a.cutoff, force, h.total);
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_grid_kernel");
	const PlanOut out = {h.plans, h.todo, h.total, h.order, h.mplans, h.ulist, h.usig, h.lists, h.segs, h.seglists};
	if (sort_n > 4096) TP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tp_linpsf_plan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sort_n * sizeof(unsigned long long))));
	TP_LAUNCH(ctx, TPK_LINPSF_PLAN, tp_linpsf_plan_kernel, dim3((unsigned)n_targets), dim3(256), (size_t)sort_n * sizeof(unsigned long long), a, out, sort_n, use_mfma, n_targets);
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_plan_kernel");
	// one round trip in the middle of the call (measured: the plan kernel's 0.2 ms and the launch of the coefficient kernel hide
	// it -- the step's wall time equals the sum of its kernels to 0.05 ms)
	TP_HIP(ctx, hipMemcpyAsync(totals, h.total, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	int64_t* c = ctx->linpsf_counts;   // tp_linpsf_last_counts
	for (int i = 0; i < 16; ++i) c[i] = 0;
	for (int k = 0; k < kMfmaClasses; ++k) {
		c[0] += (int64_t)totals[kTotClass0 + k]; c[1] += (int64_t)totals[kTotSeg0 + k];
		c[5 + k] = (int64_t)totals[kTotClass0 + k]; c[9 + k] = (int64_t)totals[kTotSeg0 + k];
	}
	c[2] = (int64_t)totals[kTotPolyTargets]; c[3] = (int64_t)totals[kTotDirectTargets];
	return TP_OK;
}

int launch_coefficients(tp_ctx* ctx, const FitArgs& a, int n_targets, const PlanScratch& h, double* d_store, double* d_kstore)
{
	const size_t coef_lds = (size_t)a.n * a.n * sizeof(double);
	TP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tp_linpsf_coef_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)coef_lds));
	TP_LAUNCH(ctx, TPK_LINPSF_COEF, tp_linpsf_coef_kernel, dim3((unsigned)n_targets), dim3(kCoefThreads), coef_lds, a, (const StarPlan*)h.plans, (const int32_t*)h.todo, d_store,
		(const MPlan*)h.mplans, (const uint16_t*)h.ulist, (const uint8_t*)h.usig, d_kstore, (const SegPlan*)h.segs);
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_coef_kernel");
	return TP_OK;
}

} // namespace tp_linpsf
