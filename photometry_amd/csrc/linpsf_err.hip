// linpsf_err.hip -- the uncertainty of the LinPSF target flux, propagated from the pixel errors (tp_linpsf_flux_err).
//
// The reference leaves flux_err NaN (linpsf_photometry.py:169, "FIXME: Add errors!") and tp_linpsf_fit reproduces that.  This pass
// is a separate entry beside the untouched fit.  Per target and cadence k, in float64:
//     good     = the pixels the fit uses: finite image value (linpsf_photometry.py:123)
//     A        = the design matrix of the fit (npx x S, :126-133): column s the pixel-integrated unit PRF of fitted star s at its
//                position of cadence k, zero outside the cut-off radius
//     G        = A^T A,  p = pinv(G)[t, :]  (t = d_target_index, numpy's rcond = 1e-15: pinv_solve with e_t as right-hand side)
//     m        = A p    (the target's flux is m . b)
//     flux_err = sqrt(sum_good (m_px * err_px)^2)
// formed in ONE pass over the pixels as  W = A^T diag(err^2) A,  var = p^T W p  -- the same number to rounding.  A non-finite err at
// a good pixel makes the cadence NaN whatever m_px is there (kept as a flag beside the sums, its err entering them as 0); a cadence
// without a good pixel gives 0 (G = W = 0), where the fit gives flux 0 as well.  A background series does not enter.
//
// One thread per cadence like tp_linpsf_fit_direct_kernel, whose walk over the pixels this is: the target's coefficient table and
// the knots in LDS, the 13 x 13 contraction per star, pixel and cadence, G and W in registers (upper triangles).  No atomics and no
// sum across lanes: a cadence's result depends on nothing but its own inputs, so two calls give the same bits and a target alone
// gives the bits it gives inside a batch.  Scaling every err by two scales W by four and the result by two, exactly.
// Targets with more than 8 fitted stars, and every target of a PRF grid that is not the SPOC layout, run with run-time sized
// G / W / V in an HBM workspace (the layout of tp_linpsf_fit_many_kernel: element e of a thread at scratch[e * n_threads + thread]).
#include "linpsf_common.h"

void* tp_ctx_scratch(tp_ctx* ctx, size_t bytes); // aperture.hip

namespace {

using namespace tp_prf;
using namespace tp_linpsf;

// 256 lanes: a wavefront may then hold 512 registers, and what the 13 x 13 contractions of two to four stars keep in flight beyond 256
// goes to the accumulation registers instead of scratch memory (with 512 lanes the 1-2 and 3-4 star classes spilled 204 / 580 bytes)
constexpr int kErrThreads = 256;
constexpr int kErrManyThreads = 256;
constexpr int kErrMaxStars = 64;

// err of pixel p of a cadence's frame (errp: its pixel 0), widened; a non-finite one raises `bad` and enters the sums as 0
__device__ __forceinline__ double fetch_err(const float* errp, int p, int64_t t_pitch, bool& bad)
{
	const float ef = errp[(int64_t)p * t_pitch];
	const bool finite = fabsf(ef) <= 3.402823466e+38f;
	bad = bad || !finite;
	return finite ? (double)ef : 0.0;
}

// p^T W p from the upper triangle of W, the diagonal term first: sum_s p_s (W_ss p_s + 2 sum_{u > s} W_su p_u)
template <int S>
__device__ __forceinline__ double quadratic_form(const double (&W)[S][S], const double (&p)[S], int ns)
{
	double var = 0.0;
#pragma unroll
	for (int s = 0; s < S; ++s) {
		if (s >= ns) continue;
		double t = 0.0;
#pragma unroll
		for (int u = 0; u < S; ++u) if (u > s && u < ns) t += W[s][u] * p[u];
		var += p[s] * (W[s][s] * p[s] + 2.0 * t);
	}
	return var;
}

// rounding can leave a variance that is zero in exact arithmetic a hair below it; a NaN stays one
__device__ __forceinline__ double err_of_variance(double var, bool bad)
{
	if (bad) return __builtin_nan("");
	return sqrt((var < 0.0) ? 0.0 : var);
}

// Up to S fitted stars out of registers (SLO..S stars: another instantiation takes the other targets), the SPOC grid.
// a.subtract is null and a.flux / a.fluxes_all are not written: only a.flux_err is.
template <int S, int SLO>
__global__ __launch_bounds__(kErrThreads) void tp_linpsf_err_kernel(FitArgs a, const float* __restrict__ images_err)
{
	extern __shared__ __align__(16) double lds[]; // [n*n] coefficient table + 2 x [n+4] knots
	const int target = blockIdx.x;
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
	const int ns = (int)(a.star_offsets[target + 1] - s0);
	const int H = a.height, W = a.width;
	const double h = kn[5] - kn[4], hy = kny[5] - kny[4];
	const double cutoff = a.cutoff;

	StarEdges<S> e;
	star_edges<S>(a, kn, kny, n, h, hy, s0, ns, k, e);

	double G[S][S], Wm[S][S];
#pragma unroll
	for (int i = 0; i < S; ++i)
#pragma unroll
		for (int j = 0; j < S; ++j) { G[i][j] = 0.0; Wm[i][j] = 0.0; }

	const float* img = a.images + (int64_t)target * H * W * a.t_pitch + k;
	const float* errp = images_err + (int64_t)target * H * W * a.t_pitch + k;
	const double h2 = h * hy;
	bool bad = false;
	for (int i = 0; i < H; ++i) {
		for (int j = 0; j < W; ++j) {
			float bf;
			if (!fetch_pixel(a, img, i * W + j, 0.f, bf)) continue;
			const double ev = fetch_err(errp, i * W + j, a.t_pitch, bad);
			const double e2 = ev * ev;
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
				const double ae = av[s] * e2;
#pragma unroll
				for (int u = 0; u < S; ++u) if (u >= s) { G[s][u] += av[s] * av[u]; Wm[s][u] += ae * av[u]; }
			}
		}
	}
#pragma unroll
	for (int s = 0; s < S; ++s)
#pragma unroll
		for (int u = 0; u < S; ++u) if (u < s) G[s][u] = G[u][s];

	const int ti = a.target_index[target];
	double et[S], p[S];
#pragma unroll
	for (int s = 0; s < S; ++s) et[s] = (s == ti) ? 1.0 : 0.0;
	pinv_solve<S>(G, et, ns, p);
	const double var = quadratic_form<S>(Wm, p, ns);
	a.flux_err[(int64_t)target * a.out_pitch + k] = (ti >= 0 && ti < ns) ? err_of_variance(var, bad) : __builtin_nan("");
}

// a thread's workspace for targets of up to S stars, in doubles: where each array starts, and their sum (the host sizes the workspace by it)
struct ErrLayout {
	int G, V, W, p, av, row, col, mx, my, ax0, by0, doubles;
	__host__ __device__ explicit ErrLayout(int S)
		: G(0), V(S * S), W(2 * S * S), p(3 * S * S), av(p + S), row(av + S), col(row + S), mx(col + S), my(mx + 4 * S), ax0(my + 4 * S), by0(ax0 + S), doubles(by0 + S) {}
};

struct ErrScratch {
	double* base; int64_t n_threads; int64_t gt;
	__device__ __forceinline__ double& at(int e) const { return base[(int64_t)e * n_threads + gt]; }
};

// Any number of stars up to smax (9 .. 64 on the SPOC grid: `targets` lists them), and with GENERAL any knot vectors, any cut-off
// radius and axes of different lengths (prf_pixel_general: the FITPACK box integral itself; `targets` null = first_target +
// blockIdx.x, the table stays in HBM when it does not fit the LDS).  Same sums in the same order as the register kernel; the
// pseudo-inverse is the cyclic Jacobi of pinv_solve, sweep order and stopping rule included, on run-time sized arrays.
template <bool GENERAL>
__global__ __launch_bounds__(kErrManyThreads) void tp_linpsf_err_many_kernel(FitArgs a, const float* __restrict__ images_err, const int32_t* __restrict__ targets,
	int first_target, int smax, double* __restrict__ scratch, int table_in_lds)
{
	extern __shared__ __align__(16) double lds[]; // [n*ny] coefficient table (if it fits) + [n+4] + [ny+4] knots
	const int target = targets ? targets[blockIdx.x] : (first_target + (int)blockIdx.x);
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
	int ns = (int)(a.star_offsets[target + 1] - s0);
	if (ns > smax) ns = smax;   // (the host sized the workspace by the largest count: never taken)
	const int H = a.height, W = a.width;
	const double h = kn[5] - kn[4], hy = kny[5] - kny[4], h2 = h * hy;
	const int S = smax;
	const ErrLayout o(S);
	ErrScratch m{scratch, (int64_t)gridDim.x * gridDim.y * blockDim.x, ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * blockDim.x + tid};
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
		for (int u = 0; u < ns; ++u) { m.at(o.G + s * S + u) = 0.0; m.at(o.W + s * S + u) = 0.0; }
	}
	const float* img = a.images + (int64_t)target * H * W * a.t_pitch + k;
	const float* errp = images_err + (int64_t)target * H * W * a.t_pitch + k;
	bool bad = false;
	for (int i = 0; i < H; ++i) {
		for (int j = 0; j < W; ++j) {
			float bf;
			if (!fetch_pixel(a, img, i * W + j, 0.f, bf)) continue;
			const double ev = fetch_err(errp, i * W + j, a.t_pitch, bad);
			const double e2 = ev * ev;
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
			if (!any) continue; // a pixel outside every cut-off disc adds nothing to G or W
			for (int s = 0; s < ns; ++s) {
				const double as = m.at(o.av + s);
				if (as == 0.0) continue;
				const double ae = as * e2;
				for (int u = s; u < ns; ++u) {
					const double au = m.at(o.av + u);
					m.at(o.G + s * S + u) += as * au;
					m.at(o.W + s * S + u) += ae * au;
				}
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
		for (int q = 0; q < ns; ++q) {
			const double d = m.at(o.G + q * S + q);
			d2 += d * d;
			for (int r = q + 1; r < ns; ++r) { const double od = m.at(o.G + q * S + r); off += od * od; }
		}
		if (!(off > 1e-34 * d2)) break;
		for (int q = 0; q < ns; ++q) {
			for (int r = q + 1; r < ns; ++r) {
				const double aqr = m.at(o.G + q * S + r);
				if (aqr == 0.0) continue;
				const double theta = (m.at(o.G + r * S + r) - m.at(o.G + q * S + q)) / (2.0 * aqr);
				const double t = ((theta >= 0.0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
				for (int e = 0; e < ns; ++e) {
					const double gq = m.at(o.G + e * S + q), gr = m.at(o.G + e * S + r);
					m.at(o.G + e * S + q) = c * gq - sn * gr;
					m.at(o.G + e * S + r) = sn * gq + c * gr;
				}
				for (int e = 0; e < ns; ++e) {
					const double gq = m.at(o.G + q * S + e), gr = m.at(o.G + r * S + e);
					m.at(o.G + q * S + e) = c * gq - sn * gr;
					m.at(o.G + r * S + e) = sn * gq + c * gr;
				}
				for (int e = 0; e < ns; ++e) {
					const double vq = m.at(o.V + e * S + q), vr = m.at(o.V + e * S + r);
					m.at(o.V + e * S + q) = c * vq - sn * vr;
					m.at(o.V + e * S + r) = sn * vq + c * vr;
				}
			}
		}
	}
	const int ti = a.target_index[target];
	const bool has_target = ti >= 0 && ti < ns;
	double smx = 0.0;
	for (int i = 0; i < ns; ++i) { const double v = fabs(m.at(o.G + i * S + i)); if (v > smx || v != v) smx = v; }
	const double cut = 1e-15 * smx;
	for (int i = 0; i < ns; ++i) m.at(o.p + i) = 0.0;
	for (int e = 0; e < ns && has_target; ++e) {
		const double lam = m.at(o.G + e * S + e);
		// (the right-hand side is e_t: the projection keeps the one term pinv_solve's sum has that is not a product with zero --
		// the zero terms are added all the same, in its order, so that the bits are those of the register kernel)
		double proj = 0.0;
		for (int i = 0; i < ns; ++i) proj += m.at(o.V + i * S + e) * ((i == ti) ? 1.0 : 0.0);
		const double inv = (fabs(lam) > cut) ? (1.0 / lam) : ((lam != lam) ? lam : 0.0);
		const double coef = proj * inv;
		for (int i = 0; i < ns; ++i) m.at(o.p + i) += m.at(o.V + i * S + e) * coef;
	}
	double var = 0.0;
	for (int s = 0; s < ns; ++s) {
		double t = 0.0;
		for (int u = s + 1; u < ns; ++u) t += m.at(o.W + s * S + u) * m.at(o.p + u);
		const double ps = m.at(o.p + s);
		var += ps * (m.at(o.W + s * S + s) * ps + 2.0 * t);
	}
	a.flux_err[(int64_t)target * a.out_pitch + k] = has_target ? err_of_variance(var, bad) : __builtin_nan("");
}

#define TP_TRY(call) do { const int _rc = (call); if (_rc != TP_OK) return _rc; } while (0)

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline size_t knots_lds(const FitArgs& a) { return ((size_t)(a.n + 4) + (size_t)(a.ny + 4)) * sizeof(double); }
inline size_t table_lds(const FitArgs& a) { return (size_t)a.n * a.ny * sizeof(double) + knots_lds(a); }
inline int many_blocks(const FitArgs& a) { return (a.n_cad + kErrManyThreads - 1) / kErrManyThreads; }
inline size_t many_scratch_per_target(const FitArgs& a, int smax) { return (size_t)ErrLayout(smax).doubles * sizeof(double) * many_blocks(a) * kErrManyThreads; }

// Can the uniform-grid kernels take this call?  The rule of tp_linpsf_grid_kernel, read off the knots on the host (two copies of
// n + 4 doubles): the SPOC layout with a cut-off whose pixel edges stay inside the evenly spaced knots.
int grid_is_uniform(tp_ctx* ctx, const FitArgs& a, bool& uniform)
{
	uniform = false;
	if (a.n != a.ny || a.n < 32 || a.n > 140 || !(a.cutoff <= 5.25)) return TP_OK;
	std::vector<double> tx((size_t)a.n + 4), ty((size_t)a.n + 4);
	TP_HIP(ctx, hipMemcpyAsync(tx.data(), a.knots_x, tx.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	TP_HIP(ctx, hipMemcpyAsync(ty.data(), a.knots_y, ty.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	uniform = uniform_grid_ok(tx.data(), a.n, a.cutoff) && uniform_grid_ok(ty.data(), a.n, a.cutoff);
	return TP_OK;
}

// the star offsets on the host (the copy synchronises the stream); no target may bring more stars than the workspace kernels take
int download_star_offsets(tp_ctx* ctx, const FitArgs& a, int n_targets, std::vector<int64_t>& off)
{
	off.resize((size_t)n_targets + 1);
	TP_HIP(ctx, hipMemcpyAsync(off.data(), a.star_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	for (int t = 0; t < n_targets; ++t) {
		const int64_t ns = off[t + 1] - off[t];
		TP_REQUIRE(ctx, ns >= 0 && ns <= kErrMaxStars, "tp_linpsf_flux_err: a target has more than 64 fitted stars");
	}
	return TP_OK;
}

template <bool GENERAL>
int launch_many(tp_ctx* ctx, const FitArgs& a, const float* d_err, const int32_t* d_list, int first, int count, int smax, double* d_scr)
{
	// (only the any-grid tables can outgrow the LDS)
	const int table_in_lds = (!GENERAL || table_lds(a) <= (size_t)160 * 1024) ? 1 : 0;
	const size_t lds = table_in_lds ? table_lds(a) : knots_lds(a);
	TP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tp_linpsf_err_many_kernel<GENERAL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	TP_LAUNCH(ctx, TPK_LINPSF_FLUX_ERR, tp_linpsf_err_many_kernel<GENERAL>, dim3((unsigned)count, (unsigned)many_blocks(a)), dim3(kErrManyThreads), lds, a, d_err, d_list, first, smax, d_scr,
		table_in_lds);
	TP_LAUNCH_CHECK(ctx, GENERAL ? "tp_linpsf_err_many_kernel (general)" : "tp_linpsf_err_many_kernel");
	return TP_OK;
}

// any grid, any cut-off: every target through the workspace kernel with the FITPACK box integral, at most 4 GiB of workspace at a time
int err_any_grid(tp_ctx* ctx, const FitArgs& a, const float* d_err, int n_targets)
{
	std::vector<int64_t> off;
	TP_TRY(download_star_offsets(ctx, a, n_targets, off));
	int smax = 1;
	for (int t = 0; t < n_targets; ++t) if ((int)(off[t + 1] - off[t]) > smax) smax = (int)(off[t + 1] - off[t]);
	const size_t per_target = many_scratch_per_target(a, smax);
	int64_t chunk = (int64_t)(((size_t)4 << 30) / per_target);
	if (chunk < 1) chunk = 1;
	if (chunk > n_targets) chunk = n_targets;
	// (the stream is idle after the download's synchronise: the scratch may move)
	TP_REQUIRE(ctx, tp_ctx_scratch(ctx, per_target * (size_t)chunk + 256) != nullptr, "tp_linpsf_flux_err: out of device memory for the workspace of the general kernel");
	double* d_scr = static_cast<double*>(ctx->scratch);
	for (int64_t first = 0; first < n_targets; first += chunk) {
		const int64_t cnt = (n_targets - first < chunk) ? (n_targets - first) : chunk;
		TP_TRY(launch_many<true>(ctx, a, d_err, nullptr, (int)first, (int)cnt, smax, d_scr));
	}
	return TP_OK;
}

// targets with more than 8 fitted stars (rare: crowded fields): listed on the host from the star offsets
int err_many_star_targets(tp_ctx* ctx, const FitArgs& a, const float* d_err, int n_targets)
{
	std::vector<int64_t> off;
	TP_TRY(download_star_offsets(ctx, a, n_targets, off));
	std::vector<int32_t> big;
	int smax = 0;
	for (int t = 0; t < n_targets; ++t) {
		const int ns = (int)(off[t + 1] - off[t]);
		if (ns > kMaxStars) { big.push_back(t); if (ns > smax) smax = ns; }
	}
	if (big.empty()) return TP_OK;
	const size_t list_bytes = align256(big.size() * sizeof(int32_t));
	const size_t per_target = many_scratch_per_target(a, smax);
	int64_t chunk = (int64_t)(((size_t)4 << 30) / per_target);
	if (chunk < 1) chunk = 1;
	if (chunk > (int64_t)big.size()) chunk = (int64_t)big.size();
	TP_REQUIRE(ctx, tp_ctx_scratch(ctx, list_bytes + per_target * (size_t)chunk + 256) != nullptr, "tp_linpsf_flux_err: out of device memory for the many-star workspace");
	char* base = static_cast<char*>(ctx->scratch);
	int32_t* d_big = reinterpret_cast<int32_t*>(base);
	TP_HIP(ctx, hipMemcpyAsync(d_big, big.data(), big.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
	for (int64_t first = 0; first < (int64_t)big.size(); first += chunk) {
		const int64_t cnt = ((int64_t)big.size() - first < chunk) ? ((int64_t)big.size() - first) : chunk;
		TP_TRY(launch_many<false>(ctx, a, d_err, d_big + first, 0, (int)cnt, smax, reinterpret_cast<double*>(base + list_bytes)));
	}
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `big` (host) must outlive the copy
	return TP_OK;
}

// one instantiation per class of star counts: a workgroup whose target belongs to another class exits at once
#define TP_LINPSF_ERR(S, SLO) do { \
	TP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tp_linpsf_err_kernel<S, SLO>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)table_lds(a))); \
	TP_LAUNCH(ctx, TPK_LINPSF_FLUX_ERR, (tp_linpsf_err_kernel<S, SLO>), grid, block, table_lds(a), a, d_err); \
	TP_LAUNCH_CHECK(ctx, "tp_linpsf_err_kernel"); } while (0)

int linpsf_err_impl(tp_ctx* ctx, const FitArgs& a, const float* d_err, int n_targets, int max_stars)
{
	bool uniform = false;
	TP_TRY(grid_is_uniform(ctx, a, uniform));
	if (!uniform) return err_any_grid(ctx, a, d_err, n_targets);
	const int nblk = (a.n_cad + kErrThreads - 1) / kErrThreads;
	const dim3 grid((unsigned)n_targets, (unsigned)nblk), block((unsigned)((((a.n_cad + nblk - 1) / nblk) + 63) / 64 * 64));
	TP_LINPSF_ERR(2, 0);
	if (max_stars > 2) TP_LINPSF_ERR(4, 3);
	if (max_stars > 4) TP_LINPSF_ERR(8, 5);
	if (max_stars > kMaxStars) TP_TRY(err_many_star_targets(ctx, a, d_err, n_targets));
	return TP_OK;
}
#undef TP_LINPSF_ERR
#undef TP_TRY

} // namespace

extern "C" int tp_linpsf_flux_err_xy(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_images_err,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis_x, int32_t n_coef_axis_y, int32_t max_stars,
	const int64_t* d_star_offsets, const int32_t* d_target_index,
	const double* d_pos_row, const double* d_pos_col, int64_t pos_pitch, double cutoff_radius,
	double* d_flux_err, int64_t out_pitch)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, tp_desc_ok(desc), "tp_linpsf_flux_err: bad cube descriptor");
	TP_REQUIRE(ctx, d_images && d_images_err && d_coef && d_knots_x && d_knots_y && d_star_offsets && d_target_index && d_pos_row && d_pos_col, "tp_linpsf_flux_err: null input pointer");
	TP_REQUIRE(ctx, d_flux_err, "tp_linpsf_flux_err: null output pointer");
	TP_REQUIRE(ctx, pos_pitch >= desc->n_cad && out_pitch >= desc->n_cad, "tp_linpsf_flux_err: pitch < n_cad");
	TP_REQUIRE(ctx, n_coef_axis_x >= 4 && n_coef_axis_x <= 2048 && n_coef_axis_y >= 4 && n_coef_axis_y <= 2048, "tp_linpsf_flux_err: coefficient table must be 4..2048 per axis");
	TP_REQUIRE(ctx, max_stars >= 1 && max_stars <= kErrMaxStars, "tp_linpsf_flux_err: at most 64 stars fitted per target");
	TP_REQUIRE(ctx, cutoff_radius > 0, "tp_linpsf_flux_err: cutoff_radius must be positive (infinity = no cut-off, psf.py:142 `cutoff_radius is None`)");
	if (desc->n_targets == 0 || desc->n_cad == 0) return TP_OK;

	FitArgs a;
	a.images = d_images; a.subtract = nullptr; a.subtract_pitch = 0;
	a.n_cad = desc->n_cad; a.height = desc->height; a.width = desc->width; a.t_pitch = desc->t_pitch;
	a.coef = d_coef; a.knots_x = d_knots_x; a.knots_y = d_knots_y; a.n = n_coef_axis_x; a.ny = n_coef_axis_y;
	a.star_offsets = d_star_offsets; a.target_index = d_target_index;
	a.pos_row = d_pos_row; a.pos_col = d_pos_col; a.pos_pitch = pos_pitch; a.cutoff = cutoff_radius;
	a.flux = nullptr; a.flux_err = d_flux_err; a.fluxes_all = nullptr; a.out_pitch = out_pitch;
	return linpsf_err_impl(ctx, a, d_images_err, (int)desc->n_targets, (int)max_stars);
	TP_API_END(ctx)
}

// the same for a square table (the SPOC PRF: 117 coefficients per axis)
extern "C" int tp_linpsf_flux_err(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_images_err,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis, int32_t max_stars,
	const int64_t* d_star_offsets, const int32_t* d_target_index,
	const double* d_pos_row, const double* d_pos_col, int64_t pos_pitch, double cutoff_radius,
	double* d_flux_err, int64_t out_pitch)
{
	return tp_linpsf_flux_err_xy(ctx, desc, d_images, d_images_err, d_coef, d_knots_x, d_knots_y, n_coef_axis, n_coef_axis, max_stars,
		d_star_offsets, d_target_index, d_pos_row, d_pos_col, pos_pitch, cutoff_radius, d_flux_err, out_pitch);
}
