// linpsf_common.h -- definitions shared by the LinPSF translation units (linpsf_plan.hip: plan / coefficient store; linpsf.hip:
// vector-ALU fit kernels, finalisers and the C entry; linpsf_mfma.hip: the matrix-core fit kernel; linpsf_err.hip: the flux errors).
// The plan's records, constants and rules are those of linpsf_plan_rules.h.
#pragma once
#include "common.h"
#include "linpsf_dev.h"
#include "linpsf_plan_rules.h"
#include <cmath>

namespace tp_linpsf {

using namespace tp_prf;

//--------------------------------------------------------------------------------------------------
// P2..P4
//--------------------------------------------------------------------------------------------------
struct FitArgs {
	const float* images; const float* subtract; int64_t subtract_pitch;
	int n_cad, height, width; int64_t t_pitch;
	const double* coef;          // [n_targets][n*n]
	const double* knots_x;       // [n+4] knots along the first spline axis (columns)
	const double* knots_y;       // [n+4] knots along the second spline axis (rows)
	int n;                       // coefficients per axis (117)
	int ny;                      // ... along the second axis (= n for every kernel but the general ones: tp_linpsf_fit_xy)
	const int64_t* star_offsets; // [n_targets+1] into the fitted-star arrays
	const int32_t* target_index; // [n_targets] index of the main target inside its fitted stars
	const double* pos_row;       // [n_fit_stars][pos_pitch] row_stamp per cadence
	const double* pos_col;       // [n_fit_stars][pos_pitch]
	int64_t pos_pitch;
	double cutoff;
	double* flux;                // [n_targets][out_pitch]  lightcurve flux (target star)
	double* flux_err;            // [n_targets][out_pitch]  NaN (linpsf_photometry.py:169)
	double* fluxes_all;          // [n_fit_stars][out_pitch] fitted flux of every star (for the mean fluxes)
	int64_t out_pitch;
};

// ---- What the direct, the many-star and the finalise kernels of linpsf.hip and the flux-error kernels of linpsf_err.hip share, each
// rule stated once.  (The build sets -ffp-contract=off:
// an expression gives the same bits in a helper as written out in a kernel.)
// pixel p of a cadence's frame (img: its pixel 0) as the fit sees it, lowered by `sub` where a.subtract is set; false unless it is
// finite: good_pixels = isfinite(img) (linpsf_photometry.py:123)
__device__ __forceinline__ bool fetch_pixel(const FitArgs& a, const float* img, int p, float sub, float& bf)
{
	bf = img[(int64_t)p * a.t_pitch];
	if (a.subtract) bf = bf - sub;
	return fabsf(bf) <= 3.402823466e+38f;
}

// psf.py:142  sqrt((j-col)^2 + (i-row)^2) < cutoff_radius  (a NaN position is never inside: zero column)
__device__ __forceinline__ bool inside_cutoff(double dc, double dr, double cutoff) { return sqrt(dc * dc + dr * dr) < cutoff; }

// the pixel-integrated PRF of a star at pixel (i, j) on the uniform grid: the table origin moved by 9 knots per pixel, clamped to the table
__device__ __forceinline__ double star_pixel_uniform(const double* __restrict__ C, int n, int ax0, int by0, int i, int j, double h2,
	const double (&mx)[4], const double (&my)[4])
{
	int ax = ax0 + 9 * j, by = by0 + 9 * i;
	ax = ax < 0 ? 0 : (ax > n - 13 ? n - 13 : ax);
	by = by < 0 ? 0 : (by > n - 13 ? n - 13 : by);
	return h2 * prf_pixel(C, n, ax, by, mx, my);
}

// the same on any grid, (dc, dr) the pixel centre: psf.py:146  integral(column_cen - 0.5, column_cen + 0.5, row_cen - 0.5, row_cen + 0.5)
__device__ __forceinline__ double star_pixel_general(const double* __restrict__ C, int n, int ny, const double* __restrict__ kn, const double* __restrict__ kny, double dc, double dr)
{ return prf_pixel_general(C, n, ny, kn, kny, dc - 0.5, dc + 0.5, dr - 0.5, dr + 0.5); }

// per register-resident star at one cadence: position, edge weights (the same for every pixel) and table origin of pixel 0
template <int S> struct StarEdges { double mx[S][4], my[S][4], srow[S], scol[S]; int ax0[S], by0[S]; };

template <int S>
__device__ __forceinline__ void star_edges(const FitArgs& a, const double* kn, const double* kny, int n, double h, double hy, int64_t s0, int ns, int k, StarEdges<S>& e)
{
#pragma unroll
	for (int s = 0; s < S; ++s) {
		if (s < ns) {
			e.srow[s] = a.pos_row[(s0 + s) * a.pos_pitch + k];
			e.scol[s] = a.pos_col[(s0 + s) * a.pos_pitch + k];
			// x <-> column (first spline axis), y <-> row  (psf.py:146)
			axis_weights(kn, n, e.scol[s], h, e.mx[s], e.ax0[s]);
			axis_weights(kny, n, e.srow[s], hy, e.my[s], e.by0[s]);
		} else {
			e.srow[s] = e.scol[s] = 0.0; e.ax0[s] = e.by0[s] = 4;
#pragma unroll
			for (int q = 0; q < 4; ++q) { e.mx[s][q] = 0.0; e.my[s][q] = 0.0; }
		}
	}
}

// Cyclic Jacobi eigen-decomposition based pseudo-inverse solve:  x = pinv(G) g,  G symmetric S x S.
template <int S>
__device__ __forceinline__ void pinv_solve(double (&G)[S][S], const double (&g)[S], int ns, double (&x)[S])
{
	double V[S][S];
#pragma unroll
	for (int i = 0; i < S; ++i)
#pragma unroll
		for (int j = 0; j < S; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
	for (int sweep = 0; sweep < 30; ++sweep) {
		double off = 0.0;
#pragma unroll
		for (int p = 0; p < S; ++p)
#pragma unroll
			for (int q = p + 1; q < S; ++q) if (q < ns) off += G[p][q] * G[p][q];
		double d2 = 0.0;
#pragma unroll
		for (int p = 0; p < S; ++p) if (p < ns) d2 += G[p][p] * G[p][p];
		if (!(off > 1e-34 * d2)) break; // off-diagonal below 1e-17 relative: converged (or NaN)
#pragma unroll
		for (int p = 0; p < S; ++p) {
#pragma unroll
			for (int q = p + 1; q < S; ++q) {
				if (q >= ns) continue;
				const double apq = G[p][q];
				if (apq == 0.0) continue;
				const double theta = (G[q][q] - G[p][p]) / (2.0 * apq);
				const double t = ((theta >= 0.0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
				for (int k = 0; k < S; ++k) {
					const double gkp = G[k][p], gkq = G[k][q];
					G[k][p] = c * gkp - s * gkq;
					G[k][q] = s * gkp + c * gkq;
				}
#pragma unroll
				for (int k = 0; k < S; ++k) {
					const double gpk = G[p][k], gqk = G[q][k];
					G[p][k] = c * gpk - s * gqk;
					G[q][k] = s * gpk + c * gqk;
				}
#pragma unroll
				for (int k = 0; k < S; ++k) {
					const double vkp = V[k][p], vkq = V[k][q];
					V[k][p] = c * vkp - s * vkq;
					V[k][q] = s * vkp + c * vkq;
				}
			}
		}
	}
	// numpy.linalg.pinv: singular values (= |eigenvalues|) <= 1e-15 * max are treated as zero
	double smax = 0.0;
#pragma unroll
	for (int i = 0; i < S; ++i) if (i < ns) { const double a = fabs(G[i][i]); if (a > smax || a != a) smax = a; }
	const double cut = 1e-15 * smax;
#pragma unroll
	for (int i = 0; i < S; ++i) x[i] = 0.0;
#pragma unroll
	for (int e = 0; e < S; ++e) {
		if (e >= ns) continue;
		const double lam = G[e][e];
		double proj = 0.0;
#pragma unroll
		for (int k = 0; k < S; ++k) if (k < ns) proj += V[k][e] * g[k];
		const double inv = (fabs(lam) > cut) ? (1.0 / lam) : ((lam != lam) ? lam : 0.0);
		const double coef = proj * inv;
#pragma unroll
		for (int k = 0; k < S; ++k) if (k < ns) x[k] += V[k][e] * coef;
	}
}


// The same solve for the well-conditioned case: Cholesky.  Returns false (x untouched) when a pivot is not safely positive
// -- singular, nearly singular or NaN normal equations -- and the caller takes pinv_solve, whose cut-off then matters
// (numpy.linalg.pinv, linpsf_photometry.py:22-34).  Where it succeeds the two agree to rounding times the condition number
// (< 1e4 here: pivots below 1e-4 of their diagonal element are refused).
template <int S>
__device__ __forceinline__ bool chol_solve(const double (&G)[S][S], const double (&g)[S], double (&x)[S])
{
	double L[S][S], y[S];
	bool ok = true;
#pragma unroll
	for (int j = 0; j < S; ++j) {
		double d = G[j][j];
#pragma unroll
		for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
		ok = ok && (d > 1e-4 * G[j][j]);
		const double inv = 1.0 / sqrt(d);
		L[j][j] = inv;   // the reciprocal of the diagonal element
#pragma unroll
		for (int i = j + 1; i < S; ++i) {
			double v = G[i][j];
#pragma unroll
			for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
			L[i][j] = v * inv;
		}
	}
	if (!ok) return false;
#pragma unroll
	for (int i = 0; i < S; ++i) {
		double v = g[i];
#pragma unroll
		for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
		y[i] = v * L[i][i];
	}
#pragma unroll
	for (int i = S - 1; i >= 0; --i) {
		double v = y[i];
#pragma unroll
		for (int k = i + 1; k < S; ++k) v -= L[k][i] * x[k];
		x[i] = v * L[i][i];
	}
	return true;
}


inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// What the plan kernel leaves for the kernels after it: the head of the context's scratch, every array on a 256-byte boundary.
// The many-star kernels' list and scratch lie behind it (`bytes` from the start).  The scratch may MOVE when it grows, and d_todo
// and d_total live in this head: so it is grown a second time only where nothing in flight or still to come reads the head -- for
// the any-grid kernels after the totals' synchronise, for the targets of more than 8 stars after a synchronise of their own.
struct PlanScratch {
	int32_t* todo; StarPlan* plans; unsigned long long* total; int32_t* order; MPlan* mplans; uint16_t* ulist; uint8_t* usig;
	int32_t* lists; SegPlan* segs; int32_t* seglists; double* alast;
	size_t todo_bytes, bytes;
};

// linpsf_plan.hip
// the arrays of the head from the address `base` on (0: only their sizes are wanted)
void carve_plan_scratch(uintptr_t base, size_t n_targets, size_t n_cad, bool with_alast, PlanScratch& h);
// Polynomial path: plan (boxes, item counts, the order of the cadences, the matrix-core lists) and the totals the host needs to
// size the store and the launches.  `use_mfma`: the matrix-core fit is on and can take this batch.
int run_plan(tp_ctx* ctx, const FitArgs& a, int n_targets, const PlanScratch& h, int use_mfma, unsigned long long (&totals)[kTotCount]);
// the coefficients of what the plan counted: polynomial items into d_store, the matrix-core images into d_kstore
int launch_coefficients(tp_ctx* ctx, const FitArgs& a, int n_targets, const PlanScratch& h, double* d_store, double* d_kstore);

// linpsf_mfma.hip
int fit_mfma_launch(tp_ctx* ctx, const FitArgs& a, int n_targets, const unsigned long long* seg_counts, const SegPlan* d_segs,
	const int32_t* d_seg_lists, const MPlan* d_mplans, const uint16_t* d_ulist, const uint8_t* d_usig, const double* d_kstore, double* d_alast);

} // namespace tp_linpsf
