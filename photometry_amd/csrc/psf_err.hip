// psf_err.hip -- the uncertainty of the PSFPhotometry light-curve flux, propagated from the pixel errors (tp_psf_flux_err).
//
// The reference leaves flux_err NaN (psf_photometry.py:175, "FIXME: Add errors!") and tp_psf_fit reproduces that.  This pass is a
// separate entry beside the untouched fit (include/tessphot_hip.h).  Per target and cadence k, in float64:
//     theta    = (row_s, col_s, f_s) of the S = min(n_fitted, 5) fitted stars, the fit's end point (d_params); a non-finite entry or
//                S = 0 gives NaN
//     w        = the fit's own float32 weights 1 / (|img + bkg| + floor), widened; good = img and w finite
//     J        = the Jacobian of the model (good x 3S): columns f_s da_s/drow_s, f_s da_s/dcol_s, a_s, with a_s the pixel-integrated
//                unit PRF (FITPACK box integral, zero outside the cut-off disc, the disc frozen at theta) and its EXACT position
//                derivatives: minus the difference of the cubic B-spline values at the pixel's edges, 0 for an edge fpintb clips
//     N        = J^T diag(w) J;  d_i = sqrt(N_ii) (1 where 0);  Ninv = D^-1 pinv(N / d d^T) D^-1  (rcond 1e-15: pinv_solve's Jacobi)
//     g        = e_{f_0} - sum_{mini and good} J_p;  q = Ninv g;  m_p = w_p (J_p . q) + [p in mini and good]
//     flux_err = sqrt(sum_good (m_p * err_p)^2): a plain sum -- a non-finite err at a good pixel gives NaN (a flag), no good pixel gives 0.
//
// Mapping (gfx950).  The cadences are independent once theta is known: one WAVEFRONT per (target, cadence), a workgroup of one
// wavefront.  Pass 1: the pixels over the lanes, each lane forms J_p and w_p of its pixels and leaves them in LDS (the coefficient
// table is read from HBM / L2 like the fit's general kernel does; the knots are in LDS).  N: its <= 120 upper-triangle entries over
// the lanes, each entry summed over the pixels in their order -- no sum across lanes at all.  The scaled pseudo-inverse: pinv_solve's
// cyclic Jacobi, same sweep order and stopping rule, on the LDS copy of N' with the element updates of a rotation spread over the
// lanes (each element is computed by the same expression as in the serial routine).  Pass 2: m_p and the sum, each lane over its
// pixels, the 64 partial sums by a fixed shuffle tree.  No atomics: two calls give the same bits, a target alone gives the bits it
// gives inside a batch, and scaling every err by two scales the result by two exactly.
// One code path for every PRF grid, table shape and cut-off (prf_pixel_general's box integral with the edge derivative).
#include "common.h"
#include "linpsf_dev.h"
#include <cmath>
#include <vector>

namespace {

using namespace tp_prf;

constexpr int kMaxPsfStars = 5;                  // psf_photometry.py:127-128 (tp_psf_fit fits the first five)
constexpr int kMaxDim = 3 * kMaxPsfStars;
constexpr int kWave = 64;
constexpr size_t kLdsLimit = 160 * 1024;

struct PsfErrArgs {
	const float* images; const float* backgrounds; const float* images_err;
	int n_cad, height, width; int64_t t_pitch;
	const double* coef; const double* knots_x; const double* knots_y; int n; int ny;
	const int64_t* star_offsets; const double* params; int64_t params_pitch; const uint8_t* mini_aperture;
	float var_floor; double cutoff;
	double* flux_err; int64_t out_pitch;
	int smax;   // the largest S of the batch: sizes a unit's LDS
};

// a unit's LDS in doubles, then bytes: where each array starts (the host sizes the launch by `bytes`)
struct ErrLds {
	size_t kn, kny, N, V, d, g, x, th, J, w, flag, bytes;
	__host__ __device__ ErrLds(int n, int ny, int P, int smax)
	{
		const size_t D = 3 * (size_t)smax;
		kn = 0; kny = kn + n + 4; N = kny + ny + 4; V = N + kMaxDim * kMaxDim; d = V + kMaxDim * kMaxDim; g = d + kMaxDim; x = g + kMaxDim;
		th = x + kMaxDim; J = th + kMaxDim; w = J + (size_t)P * D; flag = w + P;
		bytes = flag * sizeof(double) + (((size_t)P + 15) & ~(size_t)15);
	}
};

constexpr uint8_t kGood = 1, kMini = 2;

// the pixel-integrated unit PRF over [xa, xb] x [ya, yb] (prf_pixel_general, same sums in the same order) and its derivatives with
// respect to the star's column (dx) and row (dy): the limits move against the star
__device__ inline void prf_pixel_grad(const double* __restrict__ C, int n, int ny, const double* __restrict__ tx, const double* __restrict__ ty,
	double xa, double xb, double ya, double yb, double& val, double& dx, double& dy)
{
	val = dx = dy = 0.0;
	if (!(xa < xb) || !(ya < yb)) return;
	// a limit that is cut to the knot span does not move with the star
	const double uxa = (xa >= tx[3]) ? 1.0 : 0.0, uxb = (xb <= tx[n]) ? 1.0 : 0.0, uya = (ya >= ty[3]) ? 1.0 : 0.0, uyb = (yb <= ty[ny]) ? 1.0 : 0.0;
	xa = fmax(xa, tx[3]); xb = fmin(xb, tx[n]); ya = fmax(ya, ty[3]); yb = fmin(yb, ty[ny]);
	if (!(xa < xb) || !(ya < yb)) return;     // the pixel lies outside the PRF grid
	EdgeInt Xa, Xb, Ya, Yb;
	double vxa[4], vxb[4], vya[4], vyb[4];
	edge_integrals_values(tx, n, xa, Xa, vxa); edge_integrals_values(tx, n, xb, Xb, vxb);
	edge_integrals_values(ty, ny, ya, Ya, vya); edge_integrals_values(ty, ny, yb, Yb, vyb);
	for (int i = Xa.l - 3; i <= Xb.l; ++i) {
		const double wx = (edge_cumulative(Xb, i) - edge_cumulative(Xa, i)) * ((tx[i + 4] - tx[i]) * 0.25);
		const double gx = uxb * edge_value(Xb, vxb, i) - uxa * edge_value(Xa, vxa, i);
		const double* r = C + (int64_t)i * ny;
		double inner = 0.0, ginner = 0.0;
		for (int j = Ya.l - 3; j <= Yb.l; ++j) {
			const double wy = (edge_cumulative(Yb, j) - edge_cumulative(Ya, j)) * ((ty[j + 4] - ty[j]) * 0.25);
			const double gy = uyb * edge_value(Yb, vyb, j) - uya * edge_value(Ya, vya, j);
			const double c = r[j];
			inner += wy * c;
			ginner += gy * c;
		}
		val += wx * inner;
		dx += gx * inner;
		dy += wx * ginner;
	}
	dx = -dx; dy = -dy;
}

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= 3.402823466e+38f; }
__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// blockIdx.x = first_unit + target * n_cad + cadence; one wavefront
__global__ __launch_bounds__(kWave) void tp_psf_err_kernel(PsfErrArgs a, int64_t first_unit)
{
	extern __shared__ __align__(16) double lds[];
	const int64_t unit = first_unit + blockIdx.x;
	const int target = (int)(unit / a.n_cad);
	const int k = (int)(unit - (int64_t)target * a.n_cad);
	const int lane = threadIdx.x;
	const int n = a.n, ny = a.ny, H = a.height, W = a.width, P = H * W;
	const int64_t s0 = a.star_offsets[target];
	int S = (int)(a.star_offsets[target + 1] - s0);
	S = S < 0 ? 0 : (S > kMaxPsfStars ? kMaxPsfStars : S);
	if (S > a.smax) S = a.smax;   // (the host sized the LDS by the largest count: never taken)
	const int D = 3 * S;
	double* out = a.flux_err + (int64_t)target * a.out_pitch + k;

	const ErrLds o(n, ny, P, a.smax);
	double* kn = lds + o.kn; double* kny = lds + o.kny;
	double* Nm = lds + o.N; double* V = lds + o.V; double* dsc = lds + o.d; double* g = lds + o.g; double* x = lds + o.x;
	double* th = lds + o.th; double* J = lds + o.J; double* wv = lds + o.w;
	uint8_t* flag = reinterpret_cast<uint8_t*>(lds + o.flag);

	// theta through LDS; a failed fit (NaN) or nothing fitted gives NaN
	if (lane < D) th[lane] = a.params[(s0 * 3 + lane) * a.params_pitch + k];
	__syncthreads();
	bool ok = S > 0;
	for (int d = 0; d < D; ++d) ok = ok && finite64(th[d]);
	if (!ok) {   // uniform
		if (lane == 0) *out = __builtin_nan("");
		return;
	}
	for (int q = lane; q < n + 4; q += kWave) kn[q] = a.knots_x[q];
	for (int q = lane; q < ny + 4; q += kWave) kny[q] = a.knots_y[q];
	__syncthreads();

	// ---- pass 1: J_p, w_p and the flags of a lane's pixels
	const double* C = a.coef + (int64_t)target * n * ny;
	const int64_t cube = (int64_t)target * P * a.t_pitch + k;
	const uint8_t* mini = a.mini_aperture + (int64_t)target * P;
	for (int p = lane; p < P; p += kWave) {
		const float im = a.images[cube + (int64_t)p * a.t_pitch];
		const float bk = a.backgrounds ? a.backgrounds[cube + (int64_t)p * a.t_pitch] : 0.f;
		// the float32 arithmetic of tp_psf_fit_kernel (psf_photometry.py:75-86)
		float var = fabsf(im + bk) + a.var_floor;
		if (var < 1e-9f) var = 1e-9f;
		float w = 1.0f / var;
		if (w < 1e-9f) w = 1e-9f;
		const bool good = finite32(im) && finite32(w);
		flag[p] = good ? (uint8_t)(kGood | (mini[p] ? kMini : 0)) : (uint8_t)0;
		wv[p] = good ? (double)w : 0.0;
		const int i = p / W, j = p - i * W;
		double* Jp = J + (size_t)p * D;
		for (int s = 0; s < S; ++s) {
			double val = 0.0, dcol = 0.0, drow = 0.0;
			const double dc = (double)j - th[3 * s + 1], dr = (double)i - th[3 * s];
			if (good && sqrt(dc * dc + dr * dr) < a.cutoff)     // psf.py:142
				prf_pixel_grad(C, n, ny, kn, kny, dc - 0.5, dc + 0.5, dr - 0.5, dr + 0.5, val, dcol, drow);
			Jp[3 * s] = th[3 * s + 2] * drow;
			Jp[3 * s + 1] = th[3 * s + 2] * dcol;
			Jp[3 * s + 2] = val;
		}
	}
	__syncthreads();

	// ---- N = J^T diag(w) J (upper triangle, an entry per lane and turn, the pixels in their order) and g
	for (int e = lane; e < D * (D + 1) / 2; e += kWave) {
		int r = 0, c = e;
		while (c >= D - r) { c -= D - r; ++r; }
		c += r;
		double acc = 0.0;
		for (int p = 0; p < P; ++p) {
			if (!(flag[p] & kGood)) continue;
			acc += (wv[p] * J[(size_t)p * D + r]) * J[(size_t)p * D + c];
		}
		Nm[r * kMaxDim + c] = acc;
		Nm[c * kMaxDim + r] = acc;
	}
	if (lane < D) {
		double acc = 0.0;
		for (int p = 0; p < P; ++p) if (flag[p] & kMini) acc += J[(size_t)p * D + lane];
		g[lane] = ((lane == 2) ? 1.0 : 0.0) - acc;
	}
	__syncthreads();
	// ---- N' = N / (d d^T), g' = g / d, V = 1
	if (lane < D) { const double nii = Nm[lane * kMaxDim + lane]; dsc[lane] = (nii > 0.0) ? sqrt(nii) : 1.0; }
	__syncthreads();
	for (int e = lane; e < D * D; e += kWave) {
		const int r = e / D, c = e - r * D;
		Nm[r * kMaxDim + c] = Nm[r * kMaxDim + c] / (dsc[r] * dsc[c]);
		V[r * kMaxDim + c] = (r == c) ? 1.0 : 0.0;
	}
	if (lane < D) g[lane] = g[lane] / dsc[lane];
	__syncthreads();

	// ---- cyclic Jacobi (pinv_solve, linpsf_common.h: same sweep order, same stopping rule; every lane takes the same decisions on
	// values read from LDS, lane e < D updates element e of the two columns / rows a rotation touches)
	for (int sweep = 0; sweep < 30; ++sweep) {
		double off = 0.0, d2 = 0.0;
		for (int p = 0; p < D; ++p)
			for (int q = p + 1; q < D; ++q) off += Nm[p * kMaxDim + q] * Nm[p * kMaxDim + q];
		for (int p = 0; p < D; ++p) d2 += Nm[p * kMaxDim + p] * Nm[p * kMaxDim + p];
		if (!(off > 1e-34 * d2)) break;   // uniform
		for (int p = 0; p < D; ++p) {
			for (int q = p + 1; q < D; ++q) {
				const double apq = Nm[p * kMaxDim + q];
				if (apq == 0.0) continue;   // uniform
				const double theta = (Nm[q * kMaxDim + q] - Nm[p * kMaxDim + p]) / (2.0 * apq);
				const double t = ((theta >= 0.0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
				__syncthreads();   // every lane has read the pivot
				if (lane < D) {
					const double gkp = Nm[lane * kMaxDim + p], gkq = Nm[lane * kMaxDim + q];
					Nm[lane * kMaxDim + p] = c * gkp - s * gkq;
					Nm[lane * kMaxDim + q] = s * gkp + c * gkq;
					const double vkp = V[lane * kMaxDim + p], vkq = V[lane * kMaxDim + q];
					V[lane * kMaxDim + p] = c * vkp - s * vkq;
					V[lane * kMaxDim + q] = s * vkp + c * vkq;
				}
				__syncthreads();
				if (lane < D) {
					const double gpk = Nm[p * kMaxDim + lane], gqk = Nm[q * kMaxDim + lane];
					Nm[p * kMaxDim + lane] = c * gpk - s * gqk;
					Nm[q * kMaxDim + lane] = s * gpk + c * gqk;
				}
				__syncthreads();
			}
		}
	}
	// numpy.linalg.pinv: eigenvalues <= 1e-15 * max count as zero
	double smx = 0.0;
	for (int i = 0; i < D; ++i) { const double v = fabs(Nm[i * kMaxDim + i]); if (v > smx || v != v) smx = v; }
	const double cut = 1e-15 * smx;
	if (lane < D) {
		double xv = 0.0;
		for (int e = 0; e < D; ++e) {
			const double lam = Nm[e * kMaxDim + e];
			double proj = 0.0;
			for (int i = 0; i < D; ++i) proj += V[i * kMaxDim + e] * g[i];
			const double inv = (fabs(lam) > cut) ? (1.0 / lam) : ((lam != lam) ? lam : 0.0);
			xv += V[lane * kMaxDim + e] * (proj * inv);
		}
		x[lane] = xv / dsc[lane];   // q = D^-1 pinv(N') D^-1 g
	}
	__syncthreads();

	// ---- pass 2: m_p and the sum
	const float* errp = a.images_err + cube;
	double acc = 0.0;
	int bad = 0;
	for (int p = lane; p < P; p += kWave) {
		const uint8_t f = flag[p];
		if (!(f & kGood)) continue;
		const float ef = errp[(int64_t)p * a.t_pitch];
		const bool fin = finite32(ef);
		bad |= fin ? 0 : 1;
		double jq = 0.0;
		for (int d = 0; d < D; ++d) jq += J[(size_t)p * D + d] * x[d];
		const double m = wv[p] * jq + ((f & kMini) ? 1.0 : 0.0);
		const double me = m * (fin ? (double)ef : 0.0);
		acc += me * me;
	}
#pragma unroll
	for (int offs = 32; offs > 0; offs >>= 1) {
		acc += __shfl_down(acc, offs, kWave);
		bad |= __shfl_down(bad, offs, kWave);
	}
	if (lane == 0) *out = bad ? __builtin_nan("") : sqrt(acc);
}

} // namespace

extern "C" int tp_psf_flux_err_xy(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_backgrounds, const float* d_images_err,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis_x, int32_t n_coef_axis_y,
	const int64_t* d_star_offsets, const double* d_params, int64_t params_pitch, const uint8_t* d_mini_aperture,
	double variance_floor, double cutoff_radius, double* d_flux_err, int64_t out_pitch)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, tp_desc_ok(desc), "tp_psf_flux_err: bad cube descriptor");
	TP_REQUIRE(ctx, d_images && d_images_err && d_coef && d_knots_x && d_knots_y && d_star_offsets && d_params && d_mini_aperture, "tp_psf_flux_err: null input pointer");
	TP_REQUIRE(ctx, d_flux_err, "tp_psf_flux_err: null output pointer");
	TP_REQUIRE(ctx, params_pitch >= desc->n_cad && out_pitch >= desc->n_cad, "tp_psf_flux_err: pitch < n_cad");
	TP_REQUIRE(ctx, n_coef_axis_x >= 4 && n_coef_axis_x <= 2048 && n_coef_axis_y >= 4 && n_coef_axis_y <= 2048, "tp_psf_flux_err: coefficient table must be 4..2048 per axis");
	TP_REQUIRE(ctx, cutoff_radius > 0, "tp_psf_flux_err: cutoff_radius must be positive (infinity = no cut-off, psf.py:142 `cutoff_radius is None`)");
	if (desc->n_targets == 0 || desc->n_cad == 0) return TP_OK;
	// the star offsets come to the host once: the largest number of fitted stars sizes a unit's LDS
	std::vector<int64_t> off((size_t)desc->n_targets + 1);
	TP_HIP(ctx, hipMemcpyAsync(off.data(), d_star_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	int smax = 1;
	for (int t = 0; t < desc->n_targets; ++t) {
		const int64_t ns = off[(size_t)t + 1] - off[(size_t)t];
		TP_REQUIRE(ctx, ns >= 0, "tp_psf_flux_err: star offsets must not decrease");
		const int s = (int)(ns > kMaxPsfStars ? kMaxPsfStars : ns);
		if (s > smax) smax = s;
	}
	const int64_t P = (int64_t)desc->height * desc->width;
	TP_REQUIRE(ctx, P <= ((int64_t)1 << 24), "tp_psf_flux_err: stamp too large for the LDS-resident Jacobian");
	const ErrLds lds(n_coef_axis_x, n_coef_axis_y, (int)P, smax);
	TP_REQUIRE(ctx, lds.bytes <= kLdsLimit, "tp_psf_flux_err: stamp too large for the LDS-resident Jacobian");

	PsfErrArgs a;
	a.images = d_images; a.backgrounds = d_backgrounds; a.images_err = d_images_err;
	a.n_cad = desc->n_cad; a.height = desc->height; a.width = desc->width; a.t_pitch = desc->t_pitch;
	a.coef = d_coef; a.knots_x = d_knots_x; a.knots_y = d_knots_y; a.n = n_coef_axis_x; a.ny = n_coef_axis_y;
	a.star_offsets = d_star_offsets; a.params = d_params; a.params_pitch = params_pitch; a.mini_aperture = d_mini_aperture;
	a.var_floor = (float)variance_floor; a.cutoff = cutoff_radius;
	a.flux_err = d_flux_err; a.out_pitch = out_pitch; a.smax = smax;
	TP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tp_psf_err_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds.bytes));
	// one workgroup per (target, cadence), at most 2^30 of them per launch
	const int64_t units = (int64_t)desc->n_targets * desc->n_cad, chunk = (int64_t)1 << 30;
	for (int64_t first = 0; first < units; first += chunk) {
		const int64_t cnt = (units - first < chunk) ? (units - first) : chunk;
		TP_LAUNCH(ctx, TPK_PSF_FLUX_ERR, tp_psf_err_kernel, dim3((unsigned)cnt), dim3(kWave), lds.bytes, a, first);
		TP_LAUNCH_CHECK(ctx, "tp_psf_err_kernel");
	}
	return TP_OK;
	TP_API_END(ctx)
}

// the same for a square table (the SPOC PRF: 117 coefficients per axis)
extern "C" int tp_psf_flux_err(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_backgrounds, const float* d_images_err,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis,
	const int64_t* d_star_offsets, const double* d_params, int64_t params_pitch, const uint8_t* d_mini_aperture,
	double variance_floor, double cutoff_radius, double* d_flux_err, int64_t out_pitch)
{
	return tp_psf_flux_err_xy(ctx, desc, d_images, d_backgrounds, d_images_err, d_coef, d_knots_x, d_knots_y, n_coef_axis, n_coef_axis,
		d_star_offsets, d_params, params_pitch, d_mini_aperture, variance_floor, cutoff_radius, d_flux_err, out_pitch);
}
