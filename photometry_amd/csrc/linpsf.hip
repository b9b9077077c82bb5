// linpsf.hip -- P1..P4: linear PSF photometry (fixed centroids, simultaneous linear least squares).
//
// Replaces photometry/psf.py (PSF.__init__ :35-119, PSF.integrate_to_image :122-148) and
// photometry/linpsf_photometry.py (lsfit :22-34, LinPSFPhotometry.do_photometry :79-219).
//
// P1 (tp_linpsf_prf).  The reference builds, per target, PRF = sum_i PRF_i / dist_i (inverse-distance
// blend of the 25 SPOC PRF samples to the stamp centre, psf.py:101-113), normalises it (:116) and
// fits an interpolating bicubic spline (:119).  The spline fit is LINEAR in the data, so the
// coefficient table of the blend is the same blend of the 25 per-sample coefficient tables, which the
// host fits once per (camera, CCD) with the same scipy call the reference uses.  The kernel is a
// register-stationary AXPY: each thread keeps one coefficient of all samples in VGPRs and streams
// over the targets, so the base tables are read once and only the per-target table is written.
//
// P2..P4 (tp_linpsf_fit).  One THREAD per cadence of a target.  The FITPACK box integral of
// the bicubic spline over a pixel is separable (psf.py:146 -> dblint/fpintb):
//     integral = sum_ab wx[a] C[a][b] wy[b],  w = integrals of the B-spline basis over the pixel edge.
// The PRF grid is uniform (9 samples per pixel) and a pixel is exactly 9 knot intervals wide, so
// for a pixel whose lower edge sits at fraction phi of knot interval l the 13 non-zero weights are
//     [1-M(phi+3), 1-M(phi+2), 1-M(phi+1), 1-M(phi), 1, 1, 1, 1, 1, M(phi+3), M(phi+2), M(phi+1), M(phi)] * h
// with M the cumulative cardinal cubic B-spline: 4 numbers per axis per star, the same for every pixel
// of the stamp (pixels are whole multiples of 9 knots apart).  The general kernel evaluates that 13 x 13 contraction
// per star, pixel and cadence from the table in LDS; the polynomial path (below) turns it into a biquartic in the
// two phases whose 25 coefficients are shared by all cadences with the same knot intervals.
// The normal equations (A^T A, A^T b) are accumulated on the fly; x = pinv(A^T A) A^T b via a cyclic
// Jacobi eigen-decomposition with numpy's pinv cutoff (rcond = 1e-15 * largest singular value).
//
// Roofline: the FP64 pipe, not HBM: the image cube is read once (P*T*4 bytes per target).  The fit of a target
// with up to 4 stars runs on the matrix cores (linpsf_mfma.hip: ONE quartic spline per star and pixel over the knot intervals the
// star visits, cadences in natural order); the kernels of linpsf_plan.hip plan it (tp_linpsf_plan_kernel) and build its coefficients
// (tp_linpsf_coef_kernel); the kernels of this file finalise it (tp_linpsf_finalize_m_kernel) and fit the targets that do not qualify
// on the vector ALUs (tp_linpsf_fit2_kernel: a biquartic per pixel and table origin, cadences sorted by origin;
// tp_linpsf_fit_direct_kernel; tp_linpsf_fit_many_kernel).  The C entry is here.
#include "linpsf_common.h"

void* tp_ctx_scratch(tp_ctx* ctx, size_t bytes); // aperture.hip

namespace {

using namespace tp_prf;
using namespace tp_linpsf;

constexpr int kMaxSamples = 32;

//--------------------------------------------------------------------------------------------------
// P1: per-target blend of the per-sample coefficient tables
//--------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tp_linpsf_prf_kernel(const double* __restrict__ base, int n_samples, int n_coef,
	const double* __restrict__ weights, int n_targets, double* __restrict__ out)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= n_coef) return;
	double b[kMaxSamples];
#pragma unroll
	for (int s = 0; s < kMaxSamples; ++s) b[s] = (s < n_samples) ? base[(int64_t)s * n_coef + c] : 0.0;
	for (int t = blockIdx.y; t < n_targets; t += gridDim.y) {
		const double* w = weights + (int64_t)t * n_samples;
		double acc = 0.0;
#pragma unroll
		for (int s = 0; s < kMaxSamples; ++s) if (s < n_samples) acc += w[s] * b[s];
		out[(int64_t)t * n_coef + c] = acc;
	}
}

// The same for exactly NS samples (the SPOC PRF files hold 25 per CCD): with the count known the weights of a target are ONE
// batch of scalar loads (the run-time count above turns them into 25 dependent round trips: 0.67 ms for 10 000 targets against
// the 0.3 ms the 1.1 GB of tables take to write).  Same sums in the same order.
template <int NS>
__global__ __launch_bounds__(256) void tp_linpsf_prf_fixed_kernel(const double* __restrict__ base, int n_coef,
	const double* __restrict__ weights, int n_targets, double* __restrict__ out)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= n_coef) return;
	double b[NS];
#pragma unroll
	for (int s = 0; s < NS; ++s) b[s] = base[(int64_t)s * n_coef + c];
	for (int t = blockIdx.y; t < n_targets; t += gridDim.y) {
		const double* w = weights + (int64_t)t * NS;
		double wv[NS];
#pragma unroll
		for (int s = 0; s < NS; ++s) wv[s] = w[s];
		double acc = 0.0;
#pragma unroll
		for (int s = 0; s < NS; ++s) acc += wv[s] * b[s];
		out[(int64_t)t * n_coef + c] = acc;
	}
}

// (fetch_pixel, inside_cutoff, star_pixel_uniform / _general, StarEdges and star_edges live in linpsf_common.h: the flux-error pass of
// linpsf_err.hip forms the same design matrix)

// General path: direct evaluation of the 13x13 contraction per star, pixel and cadence.  Runs only for the
// targets that the polynomial path could not take (`todo` flag set, or todo == nullptr).
template <int S, int SLO>
__global__ __launch_bounds__(512) void tp_linpsf_fit_direct_kernel(FitArgs a, const int32_t* __restrict__ todo)
{
	extern __shared__ __align__(16) double lds[]; // [n*n] coefficient table + 2 x [n+4] knots
	const int target = blockIdx.x;
	if (todo && todo[target] != kPathDirect) return;
	{ const int nst = (int)(a.star_offsets[target + 1] - a.star_offsets[target]); if (nst < SLO || nst > S) return; } // another instantiation's targets
	const int tid = threadIdx.x;
	const int n = a.n;
	double* C = lds;
	double* kn = lds + (size_t)n * n;
	double* kny = kn + n + 4;
	const double* cg = a.coef + (int64_t)target * n * n;
	for (int i = tid; i < n * n; i += blockDim.x) C[i] = cg[i];
	for (int i = tid; i < n + 4; i += blockDim.x) { kn[i] = a.knots_x[i]; kny[i] = a.knots_y[i]; }
	__syncthreads();

	const int k = blockIdx.y * blockDim.x + tid;
	if (k >= a.n_cad) return;
	const int64_t s0 = a.star_offsets[target];
	int ns = (int)(a.star_offsets[target + 1] - s0);
	if (ns > S) ns = S; // host guarantees ns <= S for this instantiation
	const int H = a.height, W = a.width;
	const double h = kn[5] - kn[4], hy = kny[5] - kny[4];
	const double cutoff = a.cutoff;

	StarEdges<S> e;
	star_edges<S>(a, kn, kny, n, h, hy, s0, ns, k, e);

	double G[S][S], g[S];
#pragma unroll
	for (int i = 0; i < S; ++i) { g[i] = 0.0;
#pragma unroll
		for (int j = 0; j < S; ++j) G[i][j] = 0.0; }

	const float* img = a.images + (int64_t)target * H * W * a.t_pitch + k;
	const float sub = a.subtract ? a.subtract[(int64_t)target * a.subtract_pitch + k] : 0.f;
	const double h2 = h * hy;
	for (int i = 0; i < H; ++i) {
		for (int j = 0; j < W; ++j) {
			float bf;
			if (!fetch_pixel(a, img, i * W + j, sub, bf)) continue;
			const double b = (double)bf;
			double av[S];
#pragma unroll
			for (int s = 0; s < S; ++s) {
				av[s] = 0.0;
				if (s < ns) {
					const double dc = (double)j - e.scol[s], dr = (double)i - e.srow[s];
					if (inside_cutoff(dc, dr, cutoff)) av[s] = star_pixel_uniform(C, n, e.ax0[s], e.by0[s], i, j, h2, e.mx[s], e.my[s]);
				}
			}
#pragma unroll
			for (int s = 0; s < S; ++s) {
				g[s] += av[s] * b;
#pragma unroll
				for (int u = 0; u < S; ++u) if (u >= s) G[s][u] += av[s] * av[u];
			}
		}
	}
#pragma unroll
	for (int s = 0; s < S; ++s)
#pragma unroll
		for (int u = 0; u < S; ++u) if (u < s) G[s][u] = G[u][s];

	double x[S];
	pinv_solve<S>(G, g, ns, x);
	const int ti = a.target_index[target];
	double tf = __builtin_nan("");
#pragma unroll
	for (int s = 0; s < S; ++s) {
		if (s < ns) {
			a.fluxes_all[(s0 + s) * a.out_pitch + k] = x[s];
			if (s == ti) tf = x[s];
		}
	}
	a.flux[(int64_t)target * a.out_pitch + k] = tf;
	a.flux_err[(int64_t)target * a.out_pitch + k] = __builtin_nan("");
}

//--------------------------------------------------------------------------------------------------
// Polynomial path.  For a fixed table origin (ax0, by0) -- i.e. fixed knot intervals of the star's sub-pixel phase --
// the pixel-integrated PRF of a pixel is a BIQUARTIC polynomial of the two phases (phi_x, phi_y): the 13 edge
// weights of an axis are the quartics below.  So
//   A. per fitted star the rectangle of origins (ax0, by0) its cadences visit is found (jitter spans a few knot intervals)
//      and the coefficient table is contracted into the 25 polynomial coefficients K[a][b] of every (star, origin, pixel)
//      item (separable: 13x13 + 5x13 FMAs per column b);
//   B. every cadence evaluates its stars' PRF values by Horner (24 FMAs per star and pixel instead of 169 table reads and
//      ~230 flops) and accumulates the normal equations.
// The arithmetic differs from the direct contraction only by rounding (1e-15 relative).  A target whose stars visit more
// origins than kMaxOrigins (pointing excursions) is flagged for the general kernel.
//--------------------------------------------------------------------------------------------------
// (kEdgePoly and axis_phase live in linpsf_dev.h: the non-linear PSF kernel uses the same polynomial form)

//--------------------------------------------------------------------------------------------------
// Three kernels, plan and coef in linpsf_plan.hip (a single kernel that kept the 110 KB table in LDS, one 768-thread workgroup per CU, and read the 25
// coefficients of every Horner evaluation from LDS in every lane: 4 SIMDs share one LDS, so the coefficient reads, not the
// FMAs, set its pace -- 24 ms for the C3 batch):
//   plan  per target the boxes of its stars over ALL cadences (table origins visited, pixels that can be inside the
//         cut-off), the number of (pixel, origin) items and their place in the coefficient store (one atomic per target),
//         and the ORDER in which the fit walks the cadences: sorted by the origins of all stars (bitonic sort in LDS), because
//         the jitter straddles a knot boundary in most targets and a wavefront should see one origin per star;
//   coef  the 25 biquartic coefficients of every item, contracted from the target's table staged in LDS (one thread per
//         item, the 13 x 13 patch read once), written to the store: item = (pixel of the star's box, origin);
//   fit   one thread per cadence in 256-thread workgroups that use NO LDS: the coefficients of a (star, pixel, origin) are
//         the same for every cadence of a wavefront that sees that origin, so they are fetched by SCALAR loads from a
//         wave-uniform address (3 x s_load_dwordx16 + 1) and enter the Horner FMAs as SGPR addends (v_fma_f64 with a scalar
//         source) -- no LDS read, no barrier, and the occupancy is set by the registers.  Lanes of a wavefront that still
//         differ in origin are served in turn (ballot loop).  One instantiation per star count (1, 2, 3, 4, 5-8).
// The coefficient arithmetic and the accumulation order (pixels row-major) are those of that single kernel: same results.
// Measured (C3: 10 000 targets, 18 057 fitted stars): plan 0.65 ms, coef 1.23 ms, fit 10.9 ms (24.2 ms in the single kernel).
// Also measured: the coefficients by per-lane vector loads of one address instead of scalar loads (17.7 ms: the texture
// addresser handles 64 lanes whatever they read); natural cadence order (18.6 ms: three origins per wavefront on average);
// the cadence's pixels fetched a row ahead through LDS (13.6 against 12.5: the loop is not waiting for its pixels); two or four
// cadences per lane sharing the scalar loads and the uniform tests (10.9 - 11.9 ms for the combinations tried: no gain, the
// extra registers cost what the shared work saves).  Also: the cadences sorted by origin only inside windows of 256 / 512
// consecutive cadences (a 128-byte line of a pixel's series is then touched by one workgroup: the PMC passes show 34 GB of
// line fills per step against 12 GB of necessary bytes for the global sort): 14.2 / 12.6 ms against 10.9 -- the extra origins
// per wavefront cost more than the re-fetched lines.
//--------------------------------------------------------------------------------------------------
// a * b + c with c in scalar registers: one VOP3 instruction (left alone the compiler copies a uniform addend into vector
// registers and accumulates with v_fmac)
__device__ __forceinline__ double fma_sgpr_addend(double a, double b, double c) {
	double r;
	asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
	return r;
}

template <int S, int SLO>
__global__ __launch_bounds__(256) void tp_linpsf_fit2_kernel(FitArgs a, const StarPlan* __restrict__ plans, const int32_t* __restrict__ todo,
	const double* __restrict__ store, const int32_t* __restrict__ order)
{
	const int target = blockIdx.x;
	const int64_t s0 = a.star_offsets[target];
	int ns = (int)(a.star_offsets[target + 1] - s0);
	if (ns < SLO || ns > S) return;   // another instantiation's targets
	if (todo[target] != kPathPoly) return;   // the general / the matrix-core kernel's
	const int tid = threadIdx.x;
	const int slot = blockIdx.y * blockDim.x + tid;   // position in the origin-sorted order of the target's cadences
	const bool active = slot < a.n_cad;
	const int kreal = order[(int64_t)target * a.n_cad + (active ? slot : (a.n_cad - 1))];
	const int k = kreal;
	const int n = a.n;
	const int H = a.height, W = a.width;
	const double h = a.knots_x[5] - a.knots_x[4], hy = a.knots_y[5] - a.knots_y[4];
	const double cutoff = a.cutoff, c2 = cutoff * cutoff;

	double phx[S], phy[S], srow[S], scol[S];
	int cc[S];
	bool valid[S];
	int ncs[S], ncols[S], jmin[S], jmax[S], imin[S], imax[S];
	long long ioff[S];
	int ui0 = H, ui1 = -1, uj0 = W, uj1 = -1;
#pragma unroll
	for (int s = 0; s < S; ++s) {
		valid[s] = false; phx[s] = phy[s] = 0.0; srow[s] = scol[s] = 0.0; cc[s] = 0;
		ncs[s] = 0; ncols[s] = 0; jmin[s] = imin[s] = 0; jmax[s] = imax[s] = -1; ioff[s] = 0;
		if (s < ns) {
			const StarPlan p = plans[(int64_t)target * kMaxStars + s];
			ncs[s] = p.nc; ncols[s] = p.jmax - p.jmin + 1; jmin[s] = p.jmin; jmax[s] = p.jmax; imin[s] = p.imin; imax[s] = p.imax; ioff[s] = p.item_off;
			srow[s] = a.pos_row[(s0 + s) * a.pos_pitch + k];
			scol[s] = a.pos_col[(s0 + s) * a.pos_pitch + k];
			int ax0, by0;
			// x <-> column (first spline axis), y <-> row  (psf.py:146)
			const bool vx = axis_phase(a.knots_x, n, scol[s], h, phx[s], ax0);
			const bool vy = axis_phase(a.knots_y, n, srow[s], hy, phy[s], by0);
			valid[s] = vx && vy && (p.nc > 0);
			cc[s] = valid[s] ? ((ax0 - p.axmin) * p.nby + (by0 - p.bymin)) : 0;
			if (p.nc > 0 && p.jmax >= p.jmin && p.imax >= p.imin) {
				ui0 = (p.imin < ui0) ? p.imin : ui0; ui1 = (p.imax > ui1) ? p.imax : ui1;
				uj0 = (p.jmin < uj0) ? p.jmin : uj0; uj1 = (p.jmax > uj1) ? p.jmax : uj1;
			}
		}
	}
	double G[S][S], g[S];
#pragma unroll
	for (int s = 0; s < S; ++s) { g[s] = 0.0;
#pragma unroll
		for (int t = 0; t < S; ++t) G[s][t] = 0.0; }
	const float* img = a.images + (int64_t)target * H * W * a.t_pitch + k;
	const float sub = a.subtract ? a.subtract[(int64_t)target * a.subtract_pitch + k] : 0.f;

	// item indices relative to the target's first item: 32-bit scalar arithmetic in the pixel loop
	const double* __restrict__ tstore = store + ioff[0] * 25;
	int rel[S];
#pragma unroll
	for (int s = 0; s < S; ++s) rel[s] = (int)(ioff[s] - ioff[0]);
	for (int i = ui0; i <= ui1; ++i) {
		// per star the columns of this row that are inside the cut-off for SOME cadence of the wavefront (a float bound with a
		// margin; the exact test of psf.py:142 stays in the loop), and where the row's items start in the store
		int ja[S], jb[S], rowoff[S];
		double dr2[S];
		int jfirst = W, jend = 0;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			ja[s] = 0; jb[s] = -1; rowoff[s] = 0;
			const double dr = (double)i - srow[s];
			dr2[s] = dr * dr;
			if (s < ns && i >= imin[s] && i <= imax[s] && jmax[s] >= jmin[s]) {   // uniform
				const float w2 = (float)(c2 - dr2[s]);
				int jl = 0x3fffffff, jh = -0x3fffffff;
				if (valid[s] && w2 > -1e-3f) {
					const float w = sqrtf(fmaxf(w2, 0.f)) * 1.0001f + 1e-3f;
					jl = (int)floorf((float)scol[s] - w);
					jh = (int)ceilf((float)scol[s] + w);
				}
#pragma unroll
				for (int off = 32; off > 0; off >>= 1) {
					const int l2 = __shfl_xor(jl, off, 64), h2 = __shfl_xor(jh, off, 64);
					jl = (l2 < jl) ? l2 : jl;
					jh = (h2 > jh) ? h2 : jh;
				}
				jl = __builtin_amdgcn_readfirstlane(jl); jh = __builtin_amdgcn_readfirstlane(jh);
				ja[s] = (jl > jmin[s]) ? jl : jmin[s];
				jb[s] = (jh < jmax[s]) ? jh : jmax[s];
				rowoff[s] = rel[s] + ((i - imin[s]) * ncols[s] - jmin[s]) * ncs[s];
				if (jb[s] >= ja[s]) { jfirst = (ja[s] < jfirst) ? ja[s] : jfirst; jend = (jb[s] + 1 > jend) ? (jb[s] + 1) : jend; }
			}
		}
		if (jend <= jfirst) continue;
		auto pix_load = [&](int j) { j = (j < jend) ? j : (jend - 1); return img[((int64_t)(i * W) + j) * a.t_pitch]; };
		float pnext = pix_load(jfirst);
#pragma unroll 1
		for (int j = jfirst; j < jend; ++j) {
			const float pv = pnext;
			pnext = pix_load(j + 1);
			float bf = pv;
			if (a.subtract) bf = bf - sub;
			const bool fin = active && (fabsf(bf) <= 3.402823466e+38f);   // good_pixels = isfinite(img) (linpsf_photometry.py:123)
			const double b = (double)bf;
			double av[S];
#pragma unroll
			for (int s = 0; s < S; ++s) {
				av[s] = 0.0;
				if (j >= ja[s] && j <= jb[s]) {   // uniform
					const double dc = (double)j - scol[s];
					// psf.py:142  sqrt((j-col)^2 + (i-row)^2) < cutoff_radius; the squares decide unless they are within
					// rounding of each other (then, for the whole wavefront, the reference's own expression does)
					const double d2 = dc * dc + dr2[s];
					bool inside = d2 < c2;
					if (__any(fabs(d2 - c2) <= 1e-9 * c2)) inside = (fabs(d2 - c2) > 1e-9 * c2) ? (d2 < c2) : (sqrt(d2) < cutoff);
					const bool want = fin && valid[s] && inside;
					const int ibase = rowoff[s] + j * ncs[s];
					unsigned long long mask = __ballot(want);
					while (mask) {
						const int leader = __builtin_ctzll(mask);
						const int ccu = __builtin_amdgcn_readlane(cc[s], leader);
						const bool mine = want && (cc[s] == ccu);
						// wave-uniform address: scalar loads; the coefficients are the SGPR addends of the Horner FMAs
						const double* __restrict__ kp = tstore + (unsigned)(ibase + ccu) * 25u;
						double kc[25];
#pragma unroll
						for (int q = 0; q < 25; ++q) kc[q] = kp[q];
						double val = 0.0;
#pragma unroll
						for (int e = 4; e >= 0; --e) {
							double inner = kc[e * 5 + 4];
#pragma unroll
							for (int d = 3; d >= 0; --d) inner = fma_sgpr_addend(inner, phy[s], kc[e * 5 + d]);
							val = __builtin_fma(val, phx[s], inner);
						}
						if (mine) av[s] = val;
						mask &= ~__ballot(mine);
					}
				}
			}
			if (fin) {
#pragma unroll
				for (int s = 0; s < S; ++s) {
					g[s] += av[s] * b;
#pragma unroll
					for (int t = 0; t < S; ++t) if (t >= s) G[s][t] += av[s] * av[t];
				}
			}
		}
	}
	if (!active) return;
#pragma unroll
	for (int s = 0; s < S; ++s)
#pragma unroll
		for (int t = 0; t < S; ++t) if (t < s) G[s][t] = G[t][s];
	double x[S];
	pinv_solve<S>(G, g, ns, x);
	const int ti = a.target_index[target];
	double tf = __builtin_nan("");
#pragma unroll
	for (int s = 0; s < S; ++s) {
		if (s < ns) {
			a.fluxes_all[(s0 + s) * a.out_pitch + kreal] = x[s];
			if (s == ti) tf = x[s];
		}
	}
	a.flux[(int64_t)target * a.out_pitch + kreal] = tf;
	a.flux_err[(int64_t)target * a.out_pitch + kreal] = __builtin_nan("");
}

// Finalise (linpsf_photometry.py:197-219): mean fitted fluxes over the cadences with a valid target
// flux, contamination from the design matrix of the LAST cadence, status.
struct FinArgs {
	FitArgs f;
	double* contamination; int32_t* status; double* fluxes_mean;
	const int32_t* todo;   // targets marked kPathMfma are finalised by tp_linpsf_finalize_m_kernel (nullptr: none are)
};

constexpr int kFinThreads = 256;   // every finalise kernel: four wavefronts

// Count of the cadences with a valid target flux (returned) and the mean flux of every star over them: one pass, every thread its
// cadences in order, then a fixed tree (lanes, then the four wavefronts in order).  red: [4 * (S + 1)] in LDS, free again on return.
template <int S>
__device__ __forceinline__ double mean_fluxes(const FitArgs& a, int target, int64_t s0, int ns, double* red, double (&mean)[S])
{
	const int tid = threadIdx.x;
	const double* ftar = a.flux + (int64_t)target * a.out_pitch;
	double part[S + 1];
#pragma unroll
	for (int u = 0; u <= S; ++u) part[u] = 0.0;
	for (int k = tid; k < a.n_cad; k += kFinThreads) {
		const bool ok = ftar[k] == ftar[k];
		part[0] += ok ? 1.0 : 0.0;
#pragma unroll
		for (int s = 0; s < S; ++s) if (s < ns) { const double v = a.fluxes_all[(s0 + s) * a.out_pitch + k]; part[1 + s] += ok ? v : 0.0; }
	}
#pragma unroll
	for (int u = 0; u <= S; ++u) {
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) part[u] += __shfl_xor(part[u], off, 64);
		if ((tid & 63) == 0) red[(tid >> 6) * (S + 1) + u] = part[u];
	}
	__syncthreads();
	double cntd = 0.0;
	for (int w = 0; w < kFinThreads / 64; ++w) cntd += red[w * (S + 1)];
#pragma unroll
	for (int s = 0; s < S; ++s) {
		double tot = 0.0;
		for (int w = 0; w < kFinThreads / 64; ++w) tot += red[w * (S + 1) + 1 + s];
		mean[s] = tot / cntd;
	}
	__syncthreads();
	return cntd;
}

// A thread's `acc` summed over the workgroup by the same tree: the lanes here, then sum4 of the wavefronts' partials in red[4] (LDS).
// (A sum that starts from +0.0 is never -0.0, so adding the four partials to 0.0 in order gives the bits of sum4 too.)
__device__ __forceinline__ void wave_partials(double acc, double* red)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
	__syncthreads();
}
__device__ __forceinline__ double sum4(const double* red) { return ((red[0] + red[1]) + red[2]) + red[3]; }

// allnan(flux) -> ERROR (linpsf_photometry.py:198-200)
__device__ __forceinline__ void finish_all_nan(const FinArgs& fa, int target) { fa.status[target] = TP_STATUS_ERROR; fa.contamination[target] = __builtin_nan(""); }

// contamination = sum_p (A[p, others] . mean[others]) * A[p, target] / mean[target] (`tot`: the sum over p), the status it decides
// (linpsf_photometry.py:214-219) and the mean fluxes.  SMAX > 0: `mean` is a register array of SMAX stars (its loops must unroll);
// SMAX == 0: it lies in memory, any number of stars.
template <int SMAX>
__device__ __forceinline__ void finish_target(const FinArgs& fa, int target, double tot, int ti, int64_t s0, int ns, const double* mean)
{
	double mt = 0.0;
	if constexpr (SMAX > 0) {
#pragma unroll
		for (int u = 0; u < SMAX; ++u) if (u == ti) mt = mean[u];
	} else mt = mean[ti];
	const double cont = tot / mt;
	fa.contamination[target] = cont;
	fa.status[target] = (cont > 0.1) ? TP_STATUS_WARNING : TP_STATUS_OK;
	if (!fa.fluxes_mean) return;
	if constexpr (SMAX > 0) {
#pragma unroll
		for (int u = 0; u < SMAX; ++u) if (u < ns) fa.fluxes_mean[s0 + u] = mean[u];
	} else for (int u = 0; u < ns; ++u) fa.fluxes_mean[s0 + u] = mean[u];
}

template <int S, int SLO>
__global__ __launch_bounds__(kFinThreads) void tp_linpsf_finalize_kernel(FinArgs fa)
{
	{ const int nst = (int)(fa.f.star_offsets[blockIdx.x + 1] - fa.f.star_offsets[blockIdx.x]); if (nst < SLO || nst > S) return; } // another instantiation's targets
	if (fa.todo && fa.todo[blockIdx.x] == kPathMfma) return;
	extern __shared__ __align__(16) double lds[];
	const FitArgs& a = fa.f;
	const int target = blockIdx.x;
	const int tid = threadIdx.x;
	const int n = a.n;
	// Only the design matrix of the LAST cadence is needed (about 140 star-pixel values x 169 table entries): the table is
	// read straight from HBM / L2 instead of being staged (110 KB of LDS would allow a single workgroup per CU).
	const double* C = a.coef + (int64_t)target * n * n;
	double* kn = lds;
	double* kny = kn + n + 4;
	double* red = kny + n + 4;           // [256]
	for (int i = tid; i < n + 4; i += kFinThreads) { kn[i] = a.knots_x[i]; kny[i] = a.knots_y[i]; }
	__syncthreads();
	const int64_t s0 = a.star_offsets[target];
	int ns = (int)(a.star_offsets[target + 1] - s0);
	if (ns > S) ns = S;
	const int ti = a.target_index[target];
	double mean[S];
	const double cntd = mean_fluxes<S>(a, target, s0, ns, red, mean);
	if (cntd == 0.0) { if (tid == 0) finish_all_nan(fa, target); return; }
	const int k = a.n_cad - 1;
	const int H = a.height, W = a.width;
	const double h = kn[5] - kn[4], hy = kny[5] - kny[4], h2 = h * hy;
	StarEdges<S> e;
	star_edges<S>(a, kn, kny, n, h, hy, s0, ns, k, e);
	const float* img = a.images + (int64_t)target * H * W * a.t_pitch + k;
	const float sub = a.subtract ? a.subtract[(int64_t)target * a.subtract_pitch + k] : 0.f;
	double acc = 0.0;
	for (int p = tid; p < H * W; p += kFinThreads) {
		const int i = p / W, j = p - i * W;
		float bf;
		if (!fetch_pixel(a, img, p, sub, bf)) continue;
		double others = 0.0, at = 0.0;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			if (s >= ns) continue;
			const double dc = (double)j - e.scol[s], dr = (double)i - e.srow[s];
			double v = 0.0;
			if (inside_cutoff(dc, dr, a.cutoff)) v = star_pixel_uniform(C, n, e.ax0[s], e.by0[s], i, j, h2, e.mx[s], e.my[s]);
			if (s == ti) at = v; else others += v * mean[s];
		}
		acc += others * at;
	}
	wave_partials(acc, red);
	if (tid == 0) finish_target<S>(fa, target, sum4(red), ti, s0, ns, mean);
}

// Finalise for the targets of the matrix-core fit (class S - 1: exactly S stars): the same rules, with the design matrix of the
// last cadence as the fit kernel left it (alast[target][star][pixel of the list U], zero outside the cut-off and where the pixel
// is not finite) instead of a second evaluation of the PRF.
template <int S>
__global__ __launch_bounds__(kFinThreads) void tp_linpsf_finalize_m_kernel(FinArgs fa, const int32_t* __restrict__ targets, const MPlan* __restrict__ mplans,
	const double* __restrict__ alast)
{
	__shared__ double red[4 * (S + 1)];
	const FitArgs& a = fa.f;
	const int target = targets[blockIdx.x];
	const int tid = threadIdx.x;
	const int64_t s0 = a.star_offsets[target];
	const int ti = a.target_index[target];
	double mean[S];
	const double cntd = mean_fluxes<S>(a, target, s0, S, red, mean);
	if (cntd == 0.0) { if (tid == 0) finish_all_nan(fa, target); return; }
	const int npix = mplans[target].n_tiles * 16;
	const double* al = alast + (int64_t)target * kMfmaStars * kMfmaPixels;
	double acc = 0.0;
	for (int u = tid; u < npix; u += kFinThreads) {
		double others = 0.0, at = 0.0;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const double v = al[s * kMfmaPixels + u];
			if (s == ti) at = v; else others += v * mean[s];
		}
		acc += others * at;
	}
	wave_partials(acc, red);
	if (tid == 0) finish_target<S>(fa, target, sum4(red), ti, s0, S, mean);
}

//--------------------------------------------------------------------------------------------------
// Any number of fitted stars.  select_stars (linpsf_photometry.py:93-104) has no upper limit: a crowded target can bring
// more stars than the register-resident kernels above are instantiated for (8).  Those targets (rare) are fitted here with
// run-time sized normal equations kept in a context-owned HBM scratch: one thread per cadence like the direct kernel,
// element e of a thread's arrays at scratch[e * n_threads + thread] (coalesced across the cadences of a wavefront).
// Same arithmetic (direct 13x13 contraction, cyclic Jacobi pseudo-inverse with numpy's cut-off), only slower.
//--------------------------------------------------------------------------------------------------
constexpr int kMaxManyStars = 64;
constexpr int kManyThreads = 256;

// a thread's scratch for targets of up to S stars, in doubles: where each array starts, and their sum (the host sizes the scratch by it)
struct ManyLayout {
	int G, V, g, x, av, row, col, mx, my, ax0, by0, doubles;
	__host__ __device__ explicit ManyLayout(int S)
		: G(0), V(S * S), g(2 * S * S), x(g + S), av(x + S), row(av + S), col(row + S), mx(col + S), my(mx + 4 * S), ax0(my + 4 * S), by0(ax0 + S), doubles(by0 + S) {}
};

struct ManyScratch {
	double* base; int64_t n_threads; int64_t gt;
	__device__ __forceinline__ double& at(int e) const { return base[(int64_t)e * n_threads + gt]; }
};

// GENERAL: any knot vectors and any cut-off radius (prf_pixel_general: the FITPACK box integral itself); `big_targets` may be
// null (= every target, first_target + blockIdx.x) and the table stays in HBM when it does not fit the LDS (table_in_lds = 0).
template <bool GENERAL>
__global__ __launch_bounds__(kManyThreads) void tp_linpsf_fit_many_kernel(FitArgs a, const int32_t* __restrict__ big_targets, int first_target, int smax, double* __restrict__ scratch,
	int table_in_lds)
{
	extern __shared__ __align__(16) double lds[]; // [n*ny] coefficient table (if it fits) + [n+4] + [ny+4] knots
	const int target = big_targets ? big_targets[blockIdx.x] : (first_target + (int)blockIdx.x);
	const int tid = threadIdx.x;
	const int n = a.n, ny = a.ny;   // (ny != n only in the GENERAL instantiation)
	const double* cg = a.coef + (int64_t)target * n * ny;
	double* Cl = lds;
	double* kn = lds + (table_in_lds ? (size_t)n * ny : 0);
	double* kny = kn + n + 4;
	if (table_in_lds) for (int i = tid; i < n * ny; i += blockDim.x) Cl[i] = cg[i];
	for (int i = tid; i < n + 4; i += blockDim.x) kn[i] = a.knots_x[i];
	for (int i = tid; i < ny + 4; i += blockDim.x) kny[i] = a.knots_y[i];
	__syncthreads();
	const double* C = table_in_lds ? Cl : cg;
	const int k = blockIdx.y * blockDim.x + tid;
	if (k >= a.n_cad) return;
	const int64_t s0 = a.star_offsets[target];
	const int ns = (int)(a.star_offsets[target + 1] - s0);
	const int H = a.height, W = a.width;
	const double h = kn[5] - kn[4], hy = kny[5] - kny[4], h2 = h * hy;
	const int S = smax;
	const ManyLayout o(S);
	ManyScratch m{scratch, (int64_t)gridDim.x * gridDim.y * blockDim.x, ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * blockDim.x + tid};
	for (int s = 0; s < ns; ++s) {
		const double r = a.pos_row[(s0 + s) * a.pos_pitch + k], c = a.pos_col[(s0 + s) * a.pos_pitch + k];
		m.at(o.row + s) = r; m.at(o.col + s) = c;
		if (!GENERAL) {
			double wx[4], wy[4];
			int ax0, by0;
			axis_weights(kn, n, c, h, wx, ax0);
			axis_weights(kny, n, r, hy, wy, by0);
			for (int q = 0; q < 4; ++q) { m.at(o.mx + 4 * s + q) = wx[q]; m.at(o.my + 4 * s + q) = wy[q]; }
			m.at(o.ax0 + s) = (double)ax0; m.at(o.by0 + s) = (double)by0;
		}
		m.at(o.g + s) = 0.0;
		for (int u = 0; u < ns; ++u) m.at(o.G + s * S + u) = 0.0;
	}
	const float* img = a.images + (int64_t)target * H * W * a.t_pitch + k;
	const float sub = a.subtract ? a.subtract[(int64_t)target * a.subtract_pitch + k] : 0.f;
	for (int i = 0; i < H; ++i) {
		for (int j = 0; j < W; ++j) {
			float bf;
			if (!fetch_pixel(a, img, i * W + j, sub, bf)) continue;
			const double b = (double)bf;
			bool any = false;
			for (int s = 0; s < ns; ++s) {
				double v = 0.0;
				const double dc = (double)j - m.at(o.col + s), dr = (double)i - m.at(o.row + s);
				if (inside_cutoff(dc, dr, a.cutoff)) {
					if (GENERAL) {
						v = star_pixel_general(C, n, ny, kn, kny, dc, dr);
					} else {
						double wx[4], wy[4];
						for (int q = 0; q < 4; ++q) { wx[q] = m.at(o.mx + 4 * s + q); wy[q] = m.at(o.my + 4 * s + q); }
						v = star_pixel_uniform(C, n, (int)m.at(o.ax0 + s), (int)m.at(o.by0 + s), i, j, h2, wx, wy);
					}
					any = true;
				}
				m.at(o.av + s) = v;
			}
			if (!any) continue; // a pixel outside every cut-off disc adds nothing to A^T A or A^T b
			for (int s = 0; s < ns; ++s) {
				const double as = m.at(o.av + s);
				if (as == 0.0) continue;
				m.at(o.g + s) += as * b;
				for (int u = s; u < ns; ++u) m.at(o.G + s * S + u) += as * m.at(o.av + u);
			}
		}
	}
	for (int s = 0; s < ns; ++s) {
		for (int u = 0; u < s; ++u) m.at(o.G + s * S + u) = m.at(o.G + u * S + s);
		for (int u = 0; u < ns; ++u) m.at(o.V + s * S + u) = (s == u) ? 1.0 : 0.0;
	}
	// cyclic Jacobi (same sweep order and stopping rule as pinv_solve)
	for (int sweep = 0; sweep < 30; ++sweep) {
		double off = 0.0, d2 = 0.0;
		for (int p = 0; p < ns; ++p) {
			const double d = m.at(o.G + p * S + p);
			d2 += d * d;
			for (int q = p + 1; q < ns; ++q) { const double od = m.at(o.G + p * S + q); off += od * od; }
		}
		if (!(off > 1e-34 * d2)) break;
		for (int p = 0; p < ns; ++p) {
			for (int q = p + 1; q < ns; ++q) {
				const double apq = m.at(o.G + p * S + q);
				if (apq == 0.0) continue;
				const double theta = (m.at(o.G + q * S + q) - m.at(o.G + p * S + p)) / (2.0 * apq);
				const double t = ((theta >= 0.0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
				for (int e = 0; e < ns; ++e) {
					const double gp = m.at(o.G + e * S + p), gq = m.at(o.G + e * S + q);
					m.at(o.G + e * S + p) = c * gp - sn * gq;
					m.at(o.G + e * S + q) = sn * gp + c * gq;
				}
				for (int e = 0; e < ns; ++e) {
					const double gp = m.at(o.G + p * S + e), gq = m.at(o.G + q * S + e);
					m.at(o.G + p * S + e) = c * gp - sn * gq;
					m.at(o.G + q * S + e) = sn * gp + c * gq;
				}
				for (int e = 0; e < ns; ++e) {
					const double vp = m.at(o.V + e * S + p), vq = m.at(o.V + e * S + q);
					m.at(o.V + e * S + p) = c * vp - sn * vq;
					m.at(o.V + e * S + q) = sn * vp + c * vq;
				}
			}
		}
	}
	double smx = 0.0;
	for (int i = 0; i < ns; ++i) { const double v = fabs(m.at(o.G + i * S + i)); if (v > smx || v != v) smx = v; }
	const double cut = 1e-15 * smx;
	for (int i = 0; i < ns; ++i) m.at(o.x + i) = 0.0;
	for (int e = 0; e < ns; ++e) {
		const double lam = m.at(o.G + e * S + e);
		double proj = 0.0;
		for (int i = 0; i < ns; ++i) proj += m.at(o.V + i * S + e) * m.at(o.g + i);
		const double inv = (fabs(lam) > cut) ? (1.0 / lam) : ((lam != lam) ? lam : 0.0);
		const double coef = proj * inv;
		for (int i = 0; i < ns; ++i) m.at(o.x + i) += m.at(o.V + i * S + e) * coef;
	}
	const int ti = a.target_index[target];
	for (int s = 0; s < ns; ++s) a.fluxes_all[(s0 + s) * a.out_pitch + k] = m.at(o.x + s);
	a.flux[(int64_t)target * a.out_pitch + k] = (ti >= 0 && ti < ns) ? m.at(o.x + ti) : __builtin_nan("");
	a.flux_err[(int64_t)target * a.out_pitch + k] = __builtin_nan("");
}

// Finalise for the targets of the kernel above: the same rules, the star loops at run time, every sum serial over the 256 slots of `red`
template <bool GENERAL>
__global__ __launch_bounds__(kFinThreads) void tp_linpsf_finalize_many_kernel(FinArgs fa, const int32_t* __restrict__ big_targets, int first_target)
{
	extern __shared__ __align__(16) double lds[];
	const FitArgs& a = fa.f;
	const int target = big_targets ? big_targets[blockIdx.x] : (first_target + (int)blockIdx.x);
	const int tid = threadIdx.x;
	const int n = a.n, ny = a.ny;
	const double* C = a.coef + (int64_t)target * n * ny;
	double* kn = lds;
	double* kny = kn + n + 4;
	double* red = kny + ny + 4;           // [256]
	double* mean = red + 256;             // [kMaxManyStars]
	for (int i = tid; i < n + 4; i += blockDim.x) kn[i] = a.knots_x[i];
	for (int i = tid; i < ny + 4; i += blockDim.x) kny[i] = a.knots_y[i];
	__syncthreads();
	const int64_t s0 = a.star_offsets[target];
	const int ns = (int)(a.star_offsets[target + 1] - s0);
	const int ti = a.target_index[target];
	const double* ftar = a.flux + (int64_t)target * a.out_pitch;
	double cntd = 0.0;
	for (int s = -1; s < ns; ++s) {
		double acc = 0.0;
		for (int k = tid; k < a.n_cad; k += blockDim.x) {
			const bool ok = ftar[k] == ftar[k];
			if (s < 0) acc += ok ? 1.0 : 0.0;
			else acc += ok ? a.fluxes_all[(s0 + s) * a.out_pitch + k] : 0.0;
		}
		red[tid] = acc;
		__syncthreads();
		double tot = 0.0;
		for (int l = 0; l < (int)blockDim.x; ++l) tot += red[l];
		__syncthreads();
		if (s < 0) cntd = tot;
		else if (tid == 0) mean[s] = tot / cntd;
	}
	__syncthreads();
	if (cntd == 0.0) { if (tid == 0) finish_all_nan(fa, target); return; }
	const int k = a.n_cad - 1;
	const int H = a.height, W = a.width;
	const double h = kn[5] - kn[4], hy = kny[5] - kny[4], h2 = h * hy;
	const float* img = a.images + (int64_t)target * H * W * a.t_pitch + k;
	const float sub = a.subtract ? a.subtract[(int64_t)target * a.subtract_pitch + k] : 0.f;
	double acc = 0.0;
	for (int p = tid; p < H * W; p += blockDim.x) {
		const int i = p / W, j = p - i * W;
		float bf;
		if (!fetch_pixel(a, img, p, sub, bf)) continue;
		double others = 0.0, at = 0.0;
		for (int s = 0; s < ns; ++s) {
			const double srow = a.pos_row[(s0 + s) * a.pos_pitch + k], scol = a.pos_col[(s0 + s) * a.pos_pitch + k];
			const double dc = (double)j - scol, dr = (double)i - srow;
			double v = 0.0;
			if (inside_cutoff(dc, dr, a.cutoff)) {
				if (GENERAL) {
					v = star_pixel_general(C, n, ny, kn, kny, dc, dr);
				} else {
					double wx[4], wy[4];
					int ax0, by0;
					axis_weights(kn, n, scol, h, wx, ax0);
					axis_weights(kny, n, srow, hy, wy, by0);
					v = star_pixel_uniform(C, n, ax0, by0, i, j, h2, wx, wy);
				}
			}
			if (s == ti) at = v; else others += v * mean[s];
		}
		acc += others * at;
	}
	red[tid] = acc;
	__syncthreads();
	if (tid == 0) {
		double tot = 0.0;
		for (int l = 0; l < (int)blockDim.x; ++l) tot += red[l];
		finish_target<0>(fa, target, tot, ti, s0, ns, mean);
	}
}

} // namespace

extern "C" int tp_linpsf_prf(tp_ctx* ctx, int32_t n_targets, int32_t n_samples, int32_t n_coef,
	const double* d_base_coef, const double* d_weights, double* d_coef)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, n_targets >= 0 && n_samples > 0 && n_samples <= kMaxSamples && n_coef > 0, "tp_linpsf_prf: bad sizes (at most 32 PRF samples)");
	TP_REQUIRE(ctx, d_base_coef && d_weights && d_coef, "tp_linpsf_prf: null pointer");
	if (n_targets == 0) return TP_OK;
	const unsigned gy = (unsigned)((n_targets < 256) ? n_targets : 256);   // 54 x 256 workgroups: each thread's trip (scalar loads of the weights, 25 FMAs, one store) is a latency chain

	dim3 block(256), grid((unsigned)((n_coef + 255) / 256), gy);
	if (n_samples == 25) TP_LAUNCH(ctx, TPK_LINPSF_PRF, tp_linpsf_prf_fixed_kernel<25>, grid, block, 0, d_base_coef, (int)n_coef, d_weights, (int)n_targets, d_coef);
	else TP_LAUNCH(ctx, TPK_LINPSF_PRF, tp_linpsf_prf_kernel, grid, block, 0, d_base_coef, (int)n_samples, (int)n_coef, d_weights, (int)n_targets, d_coef);
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_prf_kernel");
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_linpsf_set_path(tp_ctx* ctx, int32_t path)
{
	TP_CHECK_CTX(ctx);
	TP_REQUIRE(ctx, path == 0 || path == 1, "tp_linpsf_set_path: 1 (matrix-core fit where a target qualifies) or 0 (vector-ALU kernels only)");
	ctx->linpsf_path = path;
	return TP_OK;
}

extern "C" int tp_linpsf_last_counts(tp_ctx* ctx, int64_t* counts, int32_t n)
{
	TP_CHECK_CTX(ctx);
	TP_REQUIRE(ctx, counts != nullptr && n >= 1 && n <= 16, "tp_linpsf_last_counts: 1..16 counters");
	for (int i = 0; i < n; ++i) counts[i] = ctx->linpsf_counts[i];
	return TP_OK;
}

namespace {

#define TP_TRY(call) do { const int _rc = (call); if (_rc != TP_OK) return _rc; } while (0)

// dynamic LDS: the knot vectors; the coefficient table before them; red[256] behind them (finalise kernels)
inline size_t knots_lds(const FitArgs& a) { return ((size_t)(a.n + 4) + (size_t)(a.ny + 4)) * sizeof(double); }
inline size_t table_lds(const FitArgs& a) { return (size_t)a.n * a.ny * sizeof(double) + knots_lds(a); }
inline size_t fin_lds(const FitArgs& a) { return knots_lds(a) + 256 * sizeof(double); }

// the star offsets on the host (the copy synchronises the stream); no target may bring more stars than the many-star kernels take
int download_star_offsets(tp_ctx* ctx, const FitArgs& a, int n_targets, std::vector<int64_t>& off)
{
	off.resize((size_t)n_targets + 1);
	TP_HIP(ctx, hipMemcpyAsync(off.data(), a.star_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	for (int t = 0; t < n_targets; ++t) {
		const int64_t ns = off[t + 1] - off[t];
		TP_REQUIRE(ctx, ns >= 0 && ns <= kMaxManyStars, "tp_linpsf_fit: a target has more than 64 fitted stars");
	}
	return TP_OK;
}

// the many-star kernels: one thread per cadence in workgroups of kManyThreads, a ManyLayout of doubles per thread
inline int many_blocks(const FitArgs& a) { return (a.n_cad + kManyThreads - 1) / kManyThreads; }
inline size_t many_scratch_per_target(const FitArgs& a, int smax) { return (size_t)ManyLayout(smax).doubles * sizeof(double) * many_blocks(a) * kManyThreads; }

// fit and finalise `count` targets of up to smax stars out of d_scr: those of d_list, or first .. first + count - 1 (d_list == nullptr)
template <bool GENERAL>
int launch_many(tp_ctx* ctx, const FitArgs& a, const FinArgs& fa, const int32_t* d_list, int first, int count, int smax, double* d_scr)
{
	// (only the any-grid tables can outgrow the LDS)
	const int table_in_lds = (!GENERAL || table_lds(a) <= (size_t)160 * 1024) ? 1 : 0;
	const size_t lds = table_in_lds ? table_lds(a) : knots_lds(a);
	TP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tp_linpsf_fit_many_kernel<GENERAL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	TP_LAUNCH(ctx, TPK_LINPSF_FIT_DIRECT, tp_linpsf_fit_many_kernel<GENERAL>, dim3((unsigned)count, (unsigned)many_blocks(a)), dim3(kManyThreads), lds, a, d_list, first, smax, d_scr, table_in_lds);
	TP_LAUNCH_CHECK(ctx, GENERAL ? "tp_linpsf_fit_many_kernel (general)" : "tp_linpsf_fit_many_kernel");
	TP_LAUNCH(ctx, TPK_LINPSF_FIN, tp_linpsf_finalize_many_kernel<GENERAL>, dim3((unsigned)count), dim3(kFinThreads), fin_lds(a) + kMaxManyStars * sizeof(double), fa, d_list, first);
	TP_LAUNCH_CHECK(ctx, GENERAL ? "tp_linpsf_finalize_many_kernel (general)" : "tp_linpsf_finalize_many_kernel");
	return TP_OK;
}

// any grid, any cut-off: every target through the run-time sized kernels with the FITPACK box integral, a few GiB of scratch at a time
int fit_any_grid(tp_ctx* ctx, const FitArgs& a, const FinArgs& fa, int n_targets, const PlanScratch& h)
{
	std::vector<int64_t> off;
	TP_TRY(download_star_offsets(ctx, a, n_targets, off));
	int smax = 1;
	for (int t = 0; t < n_targets; ++t) if ((int)(off[t + 1] - off[t]) > smax) smax = (int)(off[t + 1] - off[t]);
	const size_t per_target = many_scratch_per_target(a, smax);
	int64_t chunk = (int64_t)(((size_t)4 << 30) / per_target);
	if (chunk < 1) chunk = 1;
	if (chunk > n_targets) chunk = n_targets;
	TP_REQUIRE(ctx, tp_ctx_scratch(ctx, h.bytes + per_target * (size_t)chunk + 256) != nullptr, "tp_linpsf_fit: out of device memory for the scratch of the general kernels");
	double* d_scr = reinterpret_cast<double*>(static_cast<char*>(ctx->scratch) + h.bytes);
	for (int64_t first = 0; first < n_targets; first += chunk) {
		const int64_t cnt = (n_targets - first < chunk) ? (n_targets - first) : chunk;
		TP_TRY(launch_many<true>(ctx, a, fa, nullptr, (int)first, (int)cnt, smax, d_scr));
	}
	ctx->linpsf_counts[13] = n_targets;
	return TP_OK;
}

// targets with more than 8 fitted stars (rare: crowded fields): listed on the host from the star offsets
int fit_many_star_targets(tp_ctx* ctx, const FitArgs& a, const FinArgs& fa, int n_targets, const PlanScratch& h)
{
	std::vector<int64_t> off;
	TP_TRY(download_star_offsets(ctx, a, n_targets, off));
	std::vector<int32_t> big;
	int smax = 0;
	for (int t = 0; t < n_targets; ++t) {
		const int ns = (int)(off[t + 1] - off[t]);
		if (ns > kMaxStars) { big.push_back(t); if (ns > smax) smax = ns; }
	}
	ctx->linpsf_counts[4] = (int64_t)big.size();
	if (big.empty()) return TP_OK;
	const size_t list_bytes = align256(big.size() * sizeof(int32_t));
	const size_t need = h.bytes + list_bytes + many_scratch_per_target(a, smax) * big.size() + 256;
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the class kernels are done with the head (see PlanScratch)
	TP_REQUIRE(ctx, tp_ctx_scratch(ctx, need) != nullptr, "tp_linpsf_fit: out of device memory for the many-star scratch");
	char* base = static_cast<char*>(ctx->scratch) + h.bytes;
	int32_t* d_big = reinterpret_cast<int32_t*>(base);
	TP_HIP(ctx, hipMemcpyAsync(d_big, big.data(), big.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
	TP_TRY(launch_many<false>(ctx, a, fa, d_big, 0, (int)big.size(), smax, reinterpret_cast<double*>(base + list_bytes)));
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `big` (host) must outlive the copy
	return TP_OK;
}

// The launches of the class kernels, one instantiation per star count (the normal equations and the registers of a 1-star target are
// not those of a 4-star one); a workgroup whose target belongs to another class exits at once.  They use linpsf_fit_impl's names.
#define TP_LINPSF_FINM(S) do { if (totals[kTotClass0 + (S) - 1] > 0) { \
	TP_LAUNCH(ctx, TPK_LINPSF_FIN, (tp_linpsf_finalize_m_kernel<S>), dim3((unsigned)totals[kTotClass0 + (S) - 1]), dim3(kFinThreads), 0, fa, \
		(const int32_t*)(h.lists + (size_t)((S) - 1) * n_targets), (const MPlan*)h.mplans, (const double*)h.alast); \
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_finalize_m_kernel"); } } while (0)
#define TP_LINPSF_FIT2(S, SLO) do { \
	TP_LAUNCH(ctx, TPK_LINPSF_FIT, (tp_linpsf_fit2_kernel<S, SLO>), grid2, block2, 0, a, (const StarPlan*)h.plans, (const int32_t*)h.todo, (const double*)d_store, (const int32_t*)h.order); \
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_fit2_kernel"); } while (0)
#define TP_LINPSF_DIRECT(S, SLO) do { \
	TP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tp_linpsf_fit_direct_kernel<S, SLO>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)table_lds(a))); \
	TP_LAUNCH(ctx, TPK_LINPSF_FIT_DIRECT, (tp_linpsf_fit_direct_kernel<S, SLO>), grid, block, table_lds(a), a, (const int32_t*)h.todo); \
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_fit_direct_kernel"); \
	TP_LAUNCH(ctx, TPK_LINPSF_FIN, (tp_linpsf_finalize_kernel<S, SLO>), dim3((unsigned)n_targets), dim3(kFinThreads), fin_lds(a), fa); \
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_finalize_kernel"); } while (0)

int linpsf_fit_impl(tp_ctx* ctx, const FitArgs& a, FinArgs fa, int n_targets, int max_stars)
{
	PlanScratch h;
	carve_plan_scratch(0, (size_t)n_targets, (size_t)a.n_cad, ctx->linpsf_path == 1, h);
	TP_REQUIRE(ctx, tp_ctx_scratch(ctx, h.bytes) != nullptr, "tp_linpsf_fit: out of device memory for the plan");
	carve_plan_scratch(reinterpret_cast<uintptr_t>(ctx->scratch), (size_t)n_targets, (size_t)a.n_cad, ctx->linpsf_path == 1, h);
	// the matrix-core path needs the table in LDS (beside the 2 KB job list of its coefficient kernel), and 32-bit element offsets
	// into a target's cube
	const int use_mfma = (ctx->linpsf_path == 1 && a.n == a.ny && (size_t)a.n * a.n * sizeof(double) + 2048 <= 160 * 1024
		&& (int64_t)a.height * a.width * a.t_pitch < (1ll << 30)) ? 1 : 0;
	fa.todo = use_mfma ? h.todo : nullptr;
	unsigned long long totals[kTotCount] = {};
	TP_TRY(run_plan(ctx, a, n_targets, h, use_mfma, totals));
	if (totals[kTotGeneral] != 0) return fit_any_grid(ctx, a, fa, n_targets, h);

	// the coefficient store (polynomial items, the matrix-core images behind them), grown to what the plan counted
	const size_t poly_doubles = ((size_t)totals[kTotPolyItems] * 25 + 32 + 63) & ~(size_t)63;
	const size_t store_need = (poly_doubles + (size_t)totals[kTotKDoubles] + 64) * sizeof(double);
	if (ctx->store_bytes < store_need) {
		if (ctx->store) (void)hipFree(ctx->store);
		ctx->store = nullptr; ctx->store_bytes = 0;
		TP_HIP(ctx, tp_device_alloc(ctx, &ctx->store, store_need));
		ctx->store_bytes = store_need;
	}
	double* d_store = static_cast<double*>(ctx->store);
	double* d_kstore = d_store + poly_doubles;
	TP_TRY(launch_coefficients(ctx, a, n_targets, h, d_store, d_kstore));
	// the matrix-core fit of the targets marked for it (up to 4 stars, up to 256 reachable pixels)
	if (use_mfma) {
		TP_TRY(fit_mfma_launch(ctx, a, n_targets, totals + kTotSeg0, h.segs, h.seglists, h.mplans, h.ulist, h.usig, d_kstore, h.alast));
		TP_LINPSF_FINM(1); TP_LINPSF_FINM(2); TP_LINPSF_FINM(3); TP_LINPSF_FINM(4);
	}
	if (totals[kTotPolyTargets] > 0) {   // none when the matrix-core fit has taken every target
		const int nblk = (a.n_cad + 255) / 256;
		const dim3 grid2((unsigned)n_targets, (unsigned)nblk), block2((unsigned)((((a.n_cad + nblk - 1) / nblk) + 63) / 64 * 64));
		TP_LINPSF_FIT2(1, 0);
		if (max_stars > 1) TP_LINPSF_FIT2(2, 2);
		if (max_stars > 2) TP_LINPSF_FIT2(3, 3);
		if (max_stars > 3) TP_LINPSF_FIT2(4, 4);
		if (max_stars > 4) TP_LINPSF_FIT2(8, 5);
	}
	// the direct kernel (targets the plan flagged for it) and the finalisation of every vector-ALU target, by coarser classes
	if (totals[kTotPolyTargets] + totals[kTotDirectTargets] > 0) {
		const int nblk = (a.n_cad + 511) / 512;
		const dim3 grid((unsigned)n_targets, (unsigned)nblk), block((unsigned)((((a.n_cad + nblk - 1) / nblk) + 63) / 64 * 64));
		TP_LINPSF_DIRECT(2, 0);
		if (max_stars > 2) TP_LINPSF_DIRECT(4, 3);
		if (max_stars > 4) TP_LINPSF_DIRECT(8, 5);
	}
	if (max_stars > kMaxStars) TP_TRY(fit_many_star_targets(ctx, a, fa, n_targets, h));
	return TP_OK;
}
#undef TP_LINPSF_FINM
#undef TP_LINPSF_FIT2
#undef TP_LINPSF_DIRECT
#undef TP_TRY

} // namespace

// d_coef [n_targets][n_coef_axis_x * n_coef_axis_y], d_knots_x [n_coef_axis_x + 4], d_knots_y [n_coef_axis_y + 4]: psf.py:119 takes any
// RectBivariateSpline; a PRF spline that is not on the SPOC grid (axes of different lengths among them) is fitted by the any-grid kernels
extern "C" int tp_linpsf_fit_xy(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images,
	const float* d_subtract, int64_t subtract_pitch,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis_x, int32_t n_coef_axis_y, int32_t max_stars,
	const int64_t* d_star_offsets, const int32_t* d_target_index,
	const double* d_pos_row, const double* d_pos_col, int64_t pos_pitch, double cutoff_radius,
	double* d_flux, double* d_flux_err, double* d_fluxes_all, int64_t out_pitch,
	double* d_contamination, int32_t* d_status, double* d_fluxes_mean)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, tp_desc_ok(desc), "tp_linpsf_fit: bad cube descriptor");
	TP_REQUIRE(ctx, d_images && d_coef && d_knots_x && d_knots_y && d_star_offsets && d_target_index && d_pos_row && d_pos_col, "tp_linpsf_fit: null input pointer");
	TP_REQUIRE(ctx, d_flux && d_flux_err && d_fluxes_all && d_contamination && d_status, "tp_linpsf_fit: null output pointer");
	TP_REQUIRE(ctx, pos_pitch >= desc->n_cad && out_pitch >= desc->n_cad, "tp_linpsf_fit: pitch < n_cad");
	TP_REQUIRE(ctx, d_subtract == nullptr || subtract_pitch >= desc->n_cad, "tp_linpsf_fit: bad subtract pitch");
	TP_REQUIRE(ctx, n_coef_axis_x >= 4 && n_coef_axis_x <= 2048 && n_coef_axis_y >= 4 && n_coef_axis_y <= 2048, "tp_linpsf_fit: coefficient table must be 4..2048 per axis");
	TP_REQUIRE(ctx, max_stars >= 1 && max_stars <= kMaxManyStars, "tp_linpsf_fit: at most 64 stars fitted per target");
	TP_REQUIRE(ctx, cutoff_radius > 0, "tp_linpsf_fit: cutoff_radius must be positive (infinity = no cut-off, psf.py:142 `cutoff_radius is None`)");
	if (desc->n_targets == 0 || desc->n_cad == 0) return TP_OK;

	FitArgs a;
	a.images = d_images; a.subtract = d_subtract; a.subtract_pitch = subtract_pitch;
	a.n_cad = desc->n_cad; a.height = desc->height; a.width = desc->width; a.t_pitch = desc->t_pitch;
	a.coef = d_coef; a.knots_x = d_knots_x; a.knots_y = d_knots_y; a.n = n_coef_axis_x; a.ny = n_coef_axis_y;
	a.star_offsets = d_star_offsets; a.target_index = d_target_index;
	a.pos_row = d_pos_row; a.pos_col = d_pos_col; a.pos_pitch = pos_pitch; a.cutoff = cutoff_radius;
	a.flux = d_flux; a.flux_err = d_flux_err; a.fluxes_all = d_fluxes_all; a.out_pitch = out_pitch;
	FinArgs fa; fa.f = a; fa.contamination = d_contamination; fa.status = d_status; fa.fluxes_mean = d_fluxes_mean; fa.todo = nullptr;
	return linpsf_fit_impl(ctx, a, fa, (int)desc->n_targets, (int)max_stars);
	TP_API_END(ctx)
}

// the same for a square table (the SPOC PRF: 117 coefficients per axis)
extern "C" int tp_linpsf_fit(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images,
	const float* d_subtract, int64_t subtract_pitch,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis, int32_t max_stars,
	const int64_t* d_star_offsets, const int32_t* d_target_index,
	const double* d_pos_row, const double* d_pos_col, int64_t pos_pitch, double cutoff_radius,
	double* d_flux, double* d_flux_err, double* d_fluxes_all, int64_t out_pitch,
	double* d_contamination, int32_t* d_status, double* d_fluxes_mean)
{
	return tp_linpsf_fit_xy(ctx, desc, d_images, d_subtract, subtract_pitch, d_coef, d_knots_x, d_knots_y, n_coef_axis, n_coef_axis, max_stars,
		d_star_offsets, d_target_index, d_pos_row, d_pos_col, pos_pitch, cutoff_radius, d_flux, d_flux_err, d_fluxes_all, out_pitch,
		d_contamination, d_status, d_fluxes_mean);
}

// positions of the fitted stars of a field that moves as a whole (see tessphot_hip.h)
namespace {
__global__ __launch_bounds__(256) void tp_star_positions_kernel(int64_t n_stars, int n_cad, const float* __restrict__ base, const float* __restrict__ shift,
	double* __restrict__ pos, int64_t pitch)
{
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n_cad) return;
	const float sh = shift[k];
	for (int64_t s = blockIdx.y; s < n_stars; s += gridDim.y) pos[s * pitch + k] = (double)(base[s] + sh);
}
} // namespace

extern "C" int tp_star_positions(tp_ctx* ctx, int64_t n_stars, int32_t n_cad, const float* d_base, const float* d_shift, double* d_pos, int64_t pos_pitch)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, n_stars >= 0 && n_cad >= 0 && pos_pitch >= n_cad, "tp_star_positions: bad sizes");
	if (n_stars == 0 || n_cad == 0) return TP_OK;
	TP_REQUIRE(ctx, d_base && d_shift && d_pos, "tp_star_positions: null pointer");
	const unsigned gy = (unsigned)(n_stars < 65535 ? n_stars : 65535);
	TP_LAUNCH(ctx, TPK_STAR_POSITIONS, tp_star_positions_kernel, dim3((unsigned)((n_cad + 255) / 256), gy), dim3(256), 0, n_stars, (int)n_cad, d_base, d_shift, d_pos, pos_pitch);
	TP_LAUNCH_CHECK(ctx, "tp_star_positions_kernel");
	return TP_OK;
	TP_API_END(ctx)
}
