// motion.hip -- image movement kernels (photometry/image_motion.py): the ECC registration of a frame stack against a reference
// frame, on stacks (T, R, C) float32 resident in HBM.
//
// tp_motion_prepare: ImageMovementKernel._prepare_flux (image_motion.py:74-110) for every frame: a per-frame min / max reduction
//   (NaN ignored), then log10(flux - min + 1) rescaled to [-1, 1] and the Scharr gradient magnitude of scikit-image 0.19
//   (mode 'reflect', [1, 0, -1] along an axis then [3, 10, 3] / 16 across it, sqrt((h^2 + v^2) / 2)); NaN -> 0.  Each 1-D pass is
//   evaluated the way scipy.ndimage.correlate1d evaluates it (float64 accumulation in its order, float32 result), so the output
//   follows tests/motion_common.prepare_flux to the rounding of log10.
// tp_motion_ecc: findTransformECC (OpenCV 4.5.5, gaussFiltSize 5, all-ones mask) of every prepared frame against a prepared
//   template.  Set-up per chunk of frames: the 5 x 5 blur [1, 4, 6, 4, 1] / 16 (BORDER_REFLECT_101) of each frame.  One iteration
//   = one tile pass (the warp, bilinear with 0 outside, of the blurred frame and of its [-0.5, 0, 0.5] gradients -- recomputed from
//   the blurred frame at the four corners, so nothing but the blurred frame and the template is read -- and per-tile partial sums of
//   the raw moments N, sum I, I^2, T, T^2, IT, J_k, J_k I, J_k T, J_k J_l) plus one wave per frame that sums the partials in a fixed
//   order and does the P x P algebra (rho, lambda, delta p, the warp update, the frame's state).  No float atomics: the series is
//   bit-reproducible.  A frame that has stopped is frozen: the tile pass and the finish skip it.
// tp_motion_interpolate / tp_motion_star_positions: a loaded series of translation / euclidian / affine kernels
//   (ImageMovementKernel.load_series, image_motion.py:259-335) applied to many positions at many times (interpolate / jitter,
//   :338-421).  One thread per query time evaluates scipy's linear interp1d operation for operation (the file is compiled
//   without contraction into FMAs, so the kernels are bit-defined) and forms the cadence's 2 x 3 matrix once; the star pass
//   streams over (stars, tile of cadences) with the tile's matrices in registers, cadence the fast axis of every store.
#include "common.h"
#include <cmath>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr int kMinMaxBlocks = 64;          // min / max partials per frame
constexpr int kPrepTileC = 64, kPrepTileR = 16;
constexpr int kIterTileC = 128, kIterTileR = 32;   // 4096 pixels per tile pass block, 16 per thread

enum { ST_ACTIVE = 0, ST_CONVERGED = 1, ST_CAP = 2, ST_FAILED_NAN = 3, ST_FAILED_LAMBDA = 4 };

// scipy 'reflect' (half-sample symmetric) for a halo of one pixel
__device__ inline int reflect1(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }
// BORDER_REFLECT_101 (scipy 'mirror') for a halo of up to n - 1 pixels
__device__ inline int mirror101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ inline double wave_sum(double v) {
	for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// ---- prepare ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void tp_motion_minmax_kernel(const float* __restrict__ frames, int64_t n_pix, int64_t stride,
	float* __restrict__ part)
{
	const float* f = frames + (int64_t)blockIdx.y * stride;
	float mn = INFINITY, mx = -INFINITY;
	for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_pix; i += (int64_t)kMinMaxBlocks * kThreads) {
		const float v = f[i];
		if (v == v) { mn = fminf(mn, v); mx = fmaxf(mx, v); }
	}
	for (int o = 32; o >= 1; o >>= 1) {
		mn = fminf(mn, __shfl_xor(mn, o, 64));
		mx = fmaxf(mx, __shfl_xor(mx, o, 64));
	}
	__shared__ float smn[kThreads / 64], smx[kThreads / 64];
	if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kThreads / 64; w++) { mn = fminf(mn, smn[w]); mx = fmaxf(mx, smx[w]); }
		float* p = part + ((int64_t)blockIdx.y * kMinMaxBlocks + blockIdx.x) * 2;
		p[0] = mn;
		p[1] = mx;
	}
}

__device__ inline float log10_f32(float x) { return (float)log10((double)x); }

// grid (tiles across, tiles down, frames); block 256 = 64 columns x 4 rows, 4 output rows per thread
__global__ __launch_bounds__(kThreads) void tp_motion_prepare_kernel(const float* __restrict__ frames, int rows, int cols, int64_t stride,
	const float* __restrict__ part, float* __restrict__ out)
{
	__shared__ float s_mm[2];
	__shared__ float t[kPrepTileR + 2][kPrepTileC + 3];
	const int64_t frame = blockIdx.z;
	if (threadIdx.x < 64) {
		const float* p = part + frame * kMinMaxBlocks * 2;
		float mn = p[threadIdx.x * 2], mx = p[threadIdx.x * 2 + 1];
		for (int o = 32; o >= 1; o >>= 1) {
			mn = fminf(mn, __shfl_xor(mn, o, 64));
			mx = fmaxf(mx, __shfl_xor(mx, o, 64));
		}
		if (threadIdx.x == 0) { s_mm[0] = mn; s_mm[1] = mx; }
	}
	__syncthreads();
	const float mn = s_mm[0];
	// both transforms are monotonic: the minimum maps to log10(1) = 0, the maximum to the range (all-NaN frame: NaN throughout)
	const float ran = fabsf(log10_f32(s_mm[1] - mn + 1.0f) - 0.0f);
	const float* f = frames + frame * stride;
	const int r0 = blockIdx.y * kPrepTileR, c0 = blockIdx.x * kPrepTileC;
	for (int i = threadIdx.x; i < (kPrepTileR + 2) * (kPrepTileC + 2); i += kThreads) {
		const int tr = i / (kPrepTileC + 2), tc = i % (kPrepTileC + 2);
		const int r = reflect1(min(r0 - 1 + tr, rows), rows), c = reflect1(min(c0 - 1 + tc, cols), cols);
		const float fl = log10_f32(f[(int64_t)r * cols + c] - mn + 1.0f);
		t[tr][tc] = -1.0f + 2.0f * (float)((double)(fl - 0.0f) / (double)ran);
	}
	__syncthreads();
	const int tc = threadIdx.x & 63;
	const int c = c0 + tc;
	if (c >= cols) return;
	for (int k = threadIdx.x >> 6; k < kPrepTileR; k += kThreads / 64) {
		const int r = r0 + k;
		if (r >= rows) break;
		const int y = k + 1, x = tc + 1;
		// axis 0: [1, 0, -1] down the rows (scipy's antisymmetric form: x0 * 0 + (x[-1] - x[1]) * 1), then [3, 10, 3] / 16 across
		float d[3], e[3];
		for (int j = 0; j < 3; j++) {
			const int xx = x - 1 + j;
			d[j] = (float)((double)t[y][xx] * 0.0 + ((double)t[y - 1][xx] - (double)t[y + 1][xx]) * 1.0);
			const int yy = y - 1 + j;
			e[j] = (float)((double)t[yy][x] * 0.0 + ((double)t[yy][x - 1] - (double)t[yy][x + 1]) * 1.0);
		}
		const float h = (float)((double)d[1] * 0.625 + ((double)d[0] + (double)d[2]) * 0.1875);
		const float v = (float)((double)e[1] * 0.625 + ((double)e[0] + (double)e[2]) * 0.1875);
		const float hh = h * h, vv = v * v;
		const float s = hh + vv;
		float m = (float)sqrt((double)(s / 2.0f));
		if (m != m) m = 0.0f;
		out[frame * (int64_t)rows * cols + (int64_t)r * cols + c] = m;
	}
}

// ---- ECC set-up: the 5 x 5 blur --------------------------------------------------------------------------------------

// one correlate1d of [1, 4, 6, 4, 1] / 16 at a point (scipy's symmetric form, taps from the outside in)
__device__ inline float blur_tap(float xm2, float xm1, float x0, float xp1, float xp2) {
	double acc = (double)x0 * 0.375;
	acc += ((double)xm2 + (double)xp2) * 0.0625;
	acc += ((double)xm1 + (double)xp1) * 0.25;
	return (float)acc;
}

// grid (tiles across, tiles down, frames); in: frame i at in + index[i] * in_stride (index NULL: i); out: frame i at out + i * R * C
__global__ __launch_bounds__(kThreads) void tp_motion_blur_kernel(const float* __restrict__ in, const int32_t* __restrict__ index,
	int64_t in_stride, int rows, int cols, float* __restrict__ out)
{
	__shared__ float t[kPrepTileR + 4][kPrepTileC + 5];
	__shared__ float hrow[kPrepTileR + 4][kPrepTileC + 1];
	const int64_t frame = blockIdx.z;
	const float* f = in + (int64_t)(index ? index[frame] : frame) * in_stride;
	const int r0 = blockIdx.y * kPrepTileR, c0 = blockIdx.x * kPrepTileC;
	for (int i = threadIdx.x; i < (kPrepTileR + 4) * (kPrepTileC + 4); i += kThreads) {
		const int tr = i / (kPrepTileC + 4), tc = i % (kPrepTileC + 4);
		const int r = mirror101(min(r0 - 2 + tr, rows + 1), rows), c = mirror101(min(c0 - 2 + tc, cols + 1), cols);
		t[tr][tc] = f[(int64_t)r * cols + c];
	}
	__syncthreads();
	for (int i = threadIdx.x; i < (kPrepTileR + 4) * kPrepTileC; i += kThreads) {
		const int tr = i / kPrepTileC, tc = i % kPrepTileC;
		hrow[tr][tc] = blur_tap(t[tr][tc], t[tr][tc + 1], t[tr][tc + 2], t[tr][tc + 3], t[tr][tc + 4]);
	}
	__syncthreads();
	const int tc = threadIdx.x & 63;
	const int c = c0 + tc;
	if (c >= cols) return;
	for (int k = threadIdx.x >> 6; k < kPrepTileR; k += kThreads / 64) {
		const int r = r0 + k;
		if (r >= rows) break;
		out[frame * (int64_t)rows * cols + (int64_t)r * cols + c] = blur_tap(hrow[k][tc], hrow[k + 1][tc], hrow[k + 2][tc], hrow[k + 3][tc], hrow[k + 4][tc]);
	}
}

// ---- ECC iteration ---------------------------------------------------------------------------------------------------

template <int P> struct Acc {
	static constexpr int kJJ = P * (P + 1) / 2;
	static constexpr int K = 6 + 3 * P + kJJ;   // N, I, II, T, TT, IT, J[P], JI[P], JT[P], JJ[kJJ]
};

struct IterArgs {
	const float* blurred;      // [chunk slot][R][C]
	const float* tmpl;         // blurred template [R][C]
	const int32_t* list;       // frame ids (global) of the launch
	int32_t first;             // global id of chunk slot 0
	int rows, cols;
	int tiles_x, n_tiles;
	const double* warp;        // [n_frames][6]
	const int32_t* status;     // [n_frames]
	double* partial;           // [chunk slot][n_tiles][K]
};

// dst(x, y) = src(W [x y 1]) bilinear, 0 outside; the blurred frame's value and its two [-0.5, 0, 0.5] gradients (REFLECT_101)
__device__ inline void corner(const float* __restrict__ B, int rows, int cols, int y, int x, double& v, double& gx, double& gy) {
	if (y < 0 || y >= rows || x < 0 || x >= cols) { v = gx = gy = 0.0; return; }
	const float* row = B + (int64_t)y * cols;
	v = (double)row[x];
	const int xm = mirror101(x - 1, cols), xp = mirror101(x + 1, cols);
	const int ym = mirror101(y - 1, rows), yp = mirror101(y + 1, rows);
	gx = (double)(float)((double)row[x] * 0.0 + ((double)row[xm] - (double)row[xp]) * -0.5);
	gy = (double)(float)((double)row[x] * 0.0 + ((double)B[(int64_t)ym * cols + x] - (double)B[(int64_t)yp * cols + x]) * -0.5);
}

template <int P>
__global__ __launch_bounds__(kThreads) void tp_motion_iter_kernel(IterArgs a)
{
	constexpr int K = Acc<P>::K;
	const int f = a.list[blockIdx.y];
	if (a.status[f] != ST_ACTIVE) return;   // frozen frame (uniform over the block)
	const int slot = f - a.first;
	const float* B = a.blurred + (int64_t)slot * a.rows * a.cols;
	const double* w = a.warp + (int64_t)f * 6;
	const double w00 = w[0], w01 = w[1], w02 = w[2], w10 = w[3], w11 = w[4], w12 = w[5];
	const int tile = blockIdx.x;
	const int c0 = (tile % a.tiles_x) * kIterTileC, r0 = (tile / a.tiles_x) * kIterTileR;
	double acc[K];
#pragma unroll
	for (int k = 0; k < K; k++) acc[k] = 0.0;
	const int x = c0 + (threadIdx.x % kIterTileC);
	if (x < a.cols) {
		const double xd = (double)x;
		for (int y = r0 + (int)(threadIdx.x / kIterTileC); y < min(r0 + kIterTileR, a.rows); y += kThreads / kIterTileC) {
			const double yd = (double)y;
			const double xs = w00 * xd + w01 * yd + w02;
			const double ys = w10 * xd + w11 * yd + w12;
			// the nearest-neighbour warp of the all-ones mask (false for a non-finite warp)
			const double xn = floor(xs + 0.5), yn = floor(ys + 0.5);
			if (!(xn >= 0.0 && xn <= (double)(a.cols - 1) && yn >= 0.0 && yn <= (double)(a.rows - 1))) continue;
			const double x0d = floor(xs), y0d = floor(ys);
			const double fx = xs - x0d, fy = ys - y0d;
			const int x0 = (int)x0d, y0 = (int)y0d;   // in [-1, cols - 1] x [-1, rows - 1]
			double va, gxa, gya, vb, gxb, gyb, vc, gxc, gyc, vd, gxd, gyd;
			corner(B, a.rows, a.cols, y0, x0, va, gxa, gya);
			corner(B, a.rows, a.cols, y0, x0 + 1, vb, gxb, gyb);
			corner(B, a.rows, a.cols, y0 + 1, x0, vc, gxc, gyc);
			corner(B, a.rows, a.cols, y0 + 1, x0 + 1, vd, gxd, gyd);
			const double I = (1 - fy) * ((1 - fx) * va + fx * vb) + fy * ((1 - fx) * vc + fx * vd);
			const double gx = (1 - fy) * ((1 - fx) * gxa + fx * gxb) + fy * ((1 - fx) * gxc + fx * gxd);
			const double gy = (1 - fy) * ((1 - fx) * gya + fx * gyb) + fy * ((1 - fx) * gyc + fx * gyd);
			const double T = (double)a.tmpl[(int64_t)y * a.cols + x];
			double J[P];
			if constexpr (P == 2) {
				J[0] = gx; J[1] = gy;
			} else if constexpr (P == 3) {
				J[0] = gx * (-xd * w10 - yd * w00) + gy * (xd * w00 - yd * w10);
				J[1] = gx; J[2] = gy;
			} else {
				J[0] = gx * xd; J[1] = gy * xd; J[2] = gx * yd; J[3] = gy * yd; J[4] = gx; J[5] = gy;
			}
			acc[0] += 1.0; acc[1] += I; acc[2] += I * I; acc[3] += T; acc[4] += T * T; acc[5] += I * T;
#pragma unroll
			for (int k = 0; k < P; k++) {
				acc[6 + k] += J[k];
				acc[6 + P + k] += J[k] * I;
				acc[6 + 2 * P + k] += J[k] * T;
			}
			int q = 6 + 3 * P;
#pragma unroll
			for (int k = 0; k < P; k++)
#pragma unroll
				for (int l = k; l < P; l++) acc[q++] += J[k] * J[l];
		}
	}
	__shared__ double red[kThreads / 64][K];
#pragma unroll
	for (int k = 0; k < K; k++) {
		const double s = wave_sum(acc[k]);
		if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
	}
	__syncthreads();
	if (threadIdx.x < K) {
		double s = red[0][threadIdx.x];
		for (int wv = 1; wv < kThreads / 64; wv++) s += red[wv][threadIdx.x];
		a.partial[((int64_t)slot * a.n_tiles + tile) * K + threadIdx.x] = s;
	}
}

struct FinishArgs {
	const int32_t* list;
	int32_t first;
	int n_tiles;
	const double* partial;
	double* warp;
	double* rho;
	double* last_rho;
	int32_t* iters;
	int32_t* status;
	int32_t max_iter;
	double eps;
};

// the inverse of a symmetric positive (semi)definite P x P matrix, Gauss-Jordan with partial pivoting (the pivot row is found by
// compare-and-swap, so that every index is a compile-time constant and the matrix stays in registers); a zero pivot gives the zero
// matrix (what cv::Mat::inv returns for a singular matrix)
template <int P>
__device__ void invert(const double (&H)[P][P], double (&Hi)[P][P]) {
	double A[P][2 * P];
#pragma unroll
	for (int i = 0; i < P; i++)
#pragma unroll
		for (int j = 0; j < P; j++) { A[i][j] = H[i][j]; A[i][P + j] = i == j ? 1.0 : 0.0; }
	bool singular = false;
#pragma unroll
	for (int c = 0; c < P; c++) {
#pragma unroll
		for (int r = c + 1; r < P; r++) {
			const bool sw = fabs(A[r][c]) > fabs(A[c][c]);
#pragma unroll
			for (int j = 0; j < 2 * P; j++) {
				const double u = A[c][j], v = A[r][j];
				A[c][j] = sw ? v : u;
				A[r][j] = sw ? u : v;
			}
		}
		singular |= !(A[c][c] != 0.0);
		const double inv = 1.0 / A[c][c];
#pragma unroll
		for (int j = 0; j < 2 * P; j++) A[c][j] *= inv;
#pragma unroll
		for (int r = 0; r < P; r++) {
			if (r == c) continue;
			const double m = A[r][c];
#pragma unroll
			for (int j = 0; j < 2 * P; j++) A[r][j] -= m * A[c][j];
		}
	}
#pragma unroll
	for (int i = 0; i < P; i++)
#pragma unroll
		for (int j = 0; j < P; j++) Hi[i][j] = singular ? 0.0 : A[i][P + j];
}

// one wave per frame of the launch list
template <int P>
__global__ __launch_bounds__(64) void tp_motion_finish_kernel(FinishArgs a)
{
	constexpr int K = Acc<P>::K;
	const int f = a.list[blockIdx.x];
	if (a.status[f] != ST_ACTIVE) return;
	const double* part = a.partial + (int64_t)(f - a.first) * a.n_tiles * K;
	__shared__ double s[K];
	for (int k = 0; k < K; k++) {
		double v = 0.0;
		for (int t = threadIdx.x; t < a.n_tiles; t += 64) v += part[(int64_t)t * K + k];
		v = wave_sum(v);
		if (threadIdx.x == 0) s[k] = v;
	}
	__syncthreads();
	if (threadIdx.x != 0) return;
	const double N = s[0];
	const double muI = s[1] / N, muT = s[3] / N;
	const double imgNorm = sqrt(fmax(s[2] - s[1] * muI, 0.0));
	const double tmpNorm = sqrt(fmax(s[4] - s[3] * muT, 0.0));
	const double corr = s[5] - s[1] * muT;
	double pI[P], pT[P], H[P][P], Hi[P][P];
#pragma unroll
	for (int k = 0; k < P; k++) {
		pI[k] = s[6 + P + k] - muI * s[6 + k];
		pT[k] = s[6 + 2 * P + k] - muT * s[6 + k];
	}
	int q = 6 + 3 * P;
#pragma unroll
	for (int k = 0; k < P; k++)
#pragma unroll
		for (int l = k; l < P; l++) { H[k][l] = s[q]; H[l][k] = s[q]; q++; }
	invert<P>(H, Hi);
	const int it = a.iters[f] + 1;
	a.iters[f] = it;
	const double last = a.rho[f];
	const double rho = corr / (imgNorm * tmpNorm);
	a.last_rho[f] = last;
	a.rho[f] = rho;
	if (rho != rho) { a.status[f] = ST_FAILED_NAN; return; }
	double hpI[P];
	double pIhpI = 0.0, pThpI = 0.0;
#pragma unroll
	for (int k = 0; k < P; k++) {
		double v = 0.0;
#pragma unroll
		for (int l = 0; l < P; l++) v += Hi[k][l] * pI[l];
		hpI[k] = v;
	}
#pragma unroll
	for (int k = 0; k < P; k++) { pIhpI += pI[k] * hpI[k]; pThpI += pT[k] * hpI[k]; }
	const double lam_n = imgNorm * imgNorm - pIhpI;
	const double lam_d = corr - pThpI;
	if (lam_d <= 0.0) { a.status[f] = ST_FAILED_LAMBDA; return; }
	const double lam = lam_n / lam_d;
	double e[P], dp[P];
#pragma unroll
	for (int k = 0; k < P; k++) e[k] = lam * pT[k] - pI[k];
#pragma unroll
	for (int k = 0; k < P; k++) {
		double v = 0.0;
#pragma unroll
		for (int l = 0; l < P; l++) v += Hi[k][l] * e[l];
		dp[k] = v;
	}
	double* w = a.warp + (int64_t)f * 6;   // [w00 w01 w02 w10 w11 w12]
	if constexpr (P == 2) {
		w[2] += dp[0]; w[5] += dp[1];
	} else if constexpr (P == 3) {
		const double theta = dp[0] + asin(w[3]);
		w[2] += dp[1]; w[5] += dp[2];
		w[0] = w[4] = cos(theta);
		w[3] = sin(theta);
		w[1] = -w[3];
	} else {
		w[0] += dp[0]; w[3] += dp[1]; w[1] += dp[2]; w[4] += dp[3]; w[2] += dp[4]; w[5] += dp[5];
	}
	// the loop test of the next iteration: i <= max_iter && |rho - last_rho| >= eps
	if (!(fabs(rho - last) >= a.eps)) a.status[f] = ST_CONVERGED;
	else if (it + 1 > a.max_iter) a.status[f] = ST_CAP;
}

__global__ void tp_motion_init_kernel(int n, double* warp, double* rho, double* last_rho, int32_t* iters, int32_t* status, double eps, int32_t max_iter)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	double* w = warp + (int64_t)i * 6;
	w[0] = 1.0; w[1] = 0.0; w[2] = 0.0; w[3] = 0.0; w[4] = 1.0; w[5] = 0.0;
	rho[i] = -1.0;
	last_rho[i] = -eps;
	iters[i] = 0;
	// the loop test before the first iteration (rho = -1, last_rho = -eps)
	status[i] = !(fabs(-1.0 + eps) >= eps) ? ST_CONVERGED : (max_iter < 1 ? ST_CAP : ST_ACTIVE);
}

template <int P>
int ecc_chunks(tp_ctx* ctx, const float* d_tmpl_blur, const float* d_frames, int32_t n_frames, int32_t rows, int32_t cols, int64_t frame_stride,
	int32_t max_iter, double eps, int32_t chunk, float* d_blur, double* d_partial, int32_t* d_list, double* d_warp, double* d_rho, double* d_last,
	int32_t* d_iters, int32_t* d_status)
{
	constexpr int K = Acc<P>::K;
	const int tiles_x = (cols + kIterTileC - 1) / kIterTileC, tiles_y = (rows + kIterTileR - 1) / kIterTileR;
	const int n_tiles = tiles_x * tiles_y;
	const dim3 pgrid((unsigned)((cols + kPrepTileC - 1) / kPrepTileC), (unsigned)((rows + kPrepTileR - 1) / kPrepTileR), 1);
	std::vector<int32_t> st, list;
	for (int32_t first = 0; first < n_frames; first += chunk) {
		const int32_t n = std::min(chunk, n_frames - first);
		dim3 bgrid = pgrid;
		bgrid.z = (unsigned)n;
		TP_LAUNCH(ctx, TPK_MOTION_BLUR, tp_motion_blur_kernel, bgrid, dim3(kThreads), 0, d_frames + (int64_t)first * frame_stride, nullptr,
			frame_stride, (int)rows, (int)cols, d_blur);
		TP_LAUNCH_CHECK(ctx, "tp_motion_blur_kernel");
		list.resize(n);
		for (int i = 0; i < n; i++) list[i] = first + i;
		st.resize(n);
		int32_t n_list = n;
		int32_t done = 0;   // iterations launched for this chunk: every launch moves each active frame on by one
		int32_t poll = 4;
		while (n_list > 0 && done < max_iter) {
			TP_HIP(ctx, hipMemcpyAsync(d_list, list.data(), (size_t)n_list * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
			const int32_t steps = std::min(poll, max_iter - done);
			IterArgs ia{d_blur, d_tmpl_blur, d_list, first, (int)rows, (int)cols, tiles_x, n_tiles, d_warp, d_status, d_partial};
			FinishArgs fa{d_list, first, n_tiles, d_partial, d_warp, d_rho, d_last, d_iters, d_status, max_iter, eps};
			for (int32_t s = 0; s < steps; s++) {
				TP_LAUNCH(ctx, TPK_MOTION_ITER, tp_motion_iter_kernel<P>, dim3((unsigned)n_tiles, (unsigned)n_list), dim3(kThreads), 0, ia);
				TP_LAUNCH(ctx, TPK_MOTION_FINISH, tp_motion_finish_kernel<P>, dim3((unsigned)n_list), dim3(64), 0, fa);
			}
			TP_LAUNCH_CHECK(ctx, "tp_motion_iter_kernel");
			done += steps;
			// the frames still active: read back the states of the chunk (the host's poll of the device), relaunch over those only
			TP_HIP(ctx, hipMemcpyAsync(st.data(), d_status + first, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
			TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
			n_list = 0;
			for (int i = 0; i < n; i++) if (st[i] == ST_ACTIVE) list[n_list++] = first + i;
			poll = std::min(poll * 2, 32);
		}
	}
	(void)K;
	return TP_OK;
}

// ---- a loaded series applied to positions ---------------------------------------------------------------------------------

constexpr int kPosStars = 16;   // stars per block of the star pass: the tile's matrices are read once for all of them

// numpy's ordering of searchsorted: NaN sorts behind every number
__device__ inline bool sorts_before(double a, double b) { return a < b || (b != b && a == a); }

// One thread per query time.  kernels (may be NULL) [n_times][P]: scipy's interp1d(times, series, axis=0, assume_sorted=True,
// bounds_error=False, fill_value=(first, last)), _call_linear and _evaluate operation for operation.  mats (may be NULL)
// [6][n_times]: the rows m00 m01 m02 m10 m11 m12 of the warp of image_motion.py:147-177.
template <int P>
__global__ __launch_bounds__(kThreads) void tp_motion_interp_kernel(int n_series, const double* __restrict__ times,
	const double* __restrict__ series, const double* __restrict__ first, const double* __restrict__ last, int n_times,
	const double* __restrict__ query, double* __restrict__ kernels, double* __restrict__ mats)
{
	const int k = blockIdx.x * kThreads + threadIdx.x;
	if (k >= n_times) return;
	const double t = query[k];
	// searchsorted(times, t) (side 'left'), clipped to [1, n_series - 1]
	int lo = 0, hi = n_series;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (sorts_before(times[mid], t)) lo = mid + 1; else hi = mid;
	}
	hi = min(max(lo, 1), n_series - 1);
	lo = hi - 1;
	const double x_lo = times[lo], x_hi = times[hi];
	const bool below = t < times[0], above = t > times[n_series - 1];
	double v[P > 0 ? P : 1];
#pragma unroll
	for (int p = 0; p < P; p++) {
		const double y_lo = series[(int64_t)lo * P + p], y_hi = series[(int64_t)hi * P + p];
		const double slope = (y_hi - y_lo) / (x_hi - x_lo);
		double y = slope * (t - x_lo) + y_lo;
		if (below) y = first[p];
		if (above) y = last[p];
		v[p] = y;
		if (kernels) kernels[(int64_t)k * P + p] = y;
	}
	if (!mats) return;
	double m[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
	if constexpr (P == 2) {
		m[2] = v[0]; m[5] = v[1];
	} else if constexpr (P == 3) {
		const double c = cos(v[2]), s = sin(v[2]);
		m[0] = c; m[1] = -s; m[2] = v[0]; m[3] = s; m[4] = c; m[5] = v[1];
	} else if constexpr (P == 6) {
#pragma unroll
		for (int j = 0; j < 6; j++) m[j] = v[j];
	}
#pragma unroll
	for (int j = 0; j < 6; j++) mats[(int64_t)j * n_times + k] = m[j];
}

struct StarArgs {
	int mode, single, n_times;
	const double* mats;        // [6][n_times]
	int64_t n;
	const double* xy;          // [n][2] column, row
	const float *base_col, *base_row;
	const int64_t* out_index;
	int64_t n_out;
	double *pos_col, *pos_row;
	int64_t pitch;
	double* jitter;            // [n][n_times][2] or NULL
	int tiles;
};

// block = (chunk of kPosStars stars, tile of kThreads cadences); thread = cadence.  jitter = M [x y 1] - [x y], the products
// summed in the order of a row-times-vector loop; a translation's shift and an unchanged field's zero are copies.  single: the
// arithmetic apply_kernel does for float32 positions (np.empty_like(xy): the product is stored as float32, the position
// subtracted and the base added in float32 -- what catalog_attime gets for the float32 catalogue, BasePhotometry.py:1246-1256).
__global__ __launch_bounds__(kThreads) void tp_motion_positions_kernel(StarArgs A)
{
	const int tile = blockIdx.x % A.tiles;
	const int64_t i0 = (int64_t)(blockIdx.x / A.tiles) * kPosStars;
	const int k = tile * kThreads + threadIdx.x;
	if (k >= A.n_times) return;
	double m[6];
#pragma unroll
	for (int j = 0; j < 6; j++) m[j] = A.mats[(int64_t)j * A.n_times + k];
	const int64_t i1 = min(i0 + kPosStars, A.n);
	for (int64_t i = i0; i < i1; i++) {
		const double x = A.xy[2 * i], y = A.xy[2 * i + 1];
		double jx, jy;
		if (A.mode == TP_MOTION_UNCHANGED) {
			jx = jy = 0.0;
		} else if (A.mode == TP_MOTION_TRANSLATION) {
			jx = m[2]; jy = m[5];
			if (A.single) { jx = (double)(float)jx; jy = (double)(float)jy; }
		} else {
			const double dx = m[0] * x + m[1] * y + m[2] * 1.0;
			const double dy = m[3] * x + m[4] * y + m[5] * 1.0;
			if (A.single) {
				jx = (double)((float)dx - (float)x);
				jy = (double)((float)dy - (float)y);
			} else {
				jx = dx - x;
				jy = dy - y;
			}
		}
		if (A.jitter) {
			double* j = A.jitter + ((int64_t)i * A.n_times + k) * 2;
			j[0] = jx;
			j[1] = jy;
		}
		const int64_t o = A.n_out > 0 ? A.out_index[i] : -1;
		if (o >= 0 && o < A.n_out) {
			const float bc = A.base_col[i], br = A.base_row[i];
			if (A.single) {
				A.pos_col[o * A.pitch + k] = (double)(bc + (float)jx);
				A.pos_row[o * A.pitch + k] = (double)(br + (float)jy);
			} else {
				A.pos_col[o * A.pitch + k] = (double)(float)((double)bc + jx);
				A.pos_row[o * A.pitch + k] = (double)(float)((double)br + jy);
			}
		}
	}
}

inline int warp_params(int32_t mode) {
	return mode == TP_MOTION_UNCHANGED ? 0 : (mode == TP_MOTION_TRANSLATION ? 2 : (mode == TP_MOTION_EUCLIDIAN ? 3 : (mode == TP_MOTION_AFFINE ? 6 : -1)));
}

int launch_interp(tp_ctx* ctx, int32_t mode, int32_t n_series, const double* d_times, const double* d_series, const double* d_first,
	const double* d_last, int32_t n_times, const double* d_query, double* d_kernels, double* d_mats)
{
	const dim3 grid((unsigned)((n_times + kThreads - 1) / kThreads)), block(kThreads);
#define INTERP(P) TP_LAUNCH(ctx, TPK_MOTION_INTERP, tp_motion_interp_kernel<P>, grid, block, 0, (int)n_series, d_times, d_series, d_first, \
	d_last, (int)n_times, d_query, d_kernels, d_mats)
	switch (warp_params(mode)) {
		case 0: INTERP(0); break;
		case 2: INTERP(2); break;
		case 3: INTERP(3); break;
		default: INTERP(6); break;
	}
#undef INTERP
	TP_LAUNCH_CHECK(ctx, "tp_motion_interp_kernel");
	return TP_OK;
}

} // namespace

extern "C" int tp_motion_prepare(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	float* d_out)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, d_frames && d_out && d_frames != d_out, "tp_motion_prepare: null or aliased pointers");
	TP_REQUIRE(ctx, n_frames >= 0 && n_frames <= 65535 && frame_rows >= 3 && frame_cols >= 3 && frame_stride >= (int64_t)frame_rows * frame_cols,
		"tp_motion_prepare: bad frame geometry");
	if (n_frames == 0) return TP_OK;
	const int64_t n_pix = (int64_t)frame_rows * frame_cols;
	float* part = nullptr;
	const int rc = tp_malloc(ctx, (uint64_t)n_frames * kMinMaxBlocks * 2 * sizeof(float), (void**)&part);
	if (rc != TP_OK) return rc;
	TP_LAUNCH(ctx, TPK_MOTION_MINMAX, tp_motion_minmax_kernel, dim3(kMinMaxBlocks, (unsigned)n_frames), dim3(kThreads), 0, d_frames, n_pix, frame_stride, part);
	const dim3 grid((unsigned)((frame_cols + kPrepTileC - 1) / kPrepTileC), (unsigned)((frame_rows + kPrepTileR - 1) / kPrepTileR), (unsigned)n_frames);
	TP_LAUNCH(ctx, TPK_MOTION_PREPARE, tp_motion_prepare_kernel, grid, dim3(kThreads), 0, d_frames, (int)frame_rows, (int)frame_cols, frame_stride, part, d_out);
	tp_free(ctx, part);
	TP_LAUNCH_CHECK(ctx, "tp_motion_prepare_kernel");
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_motion_ecc(tp_ctx* ctx, const float* d_template, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t frame_stride, int32_t n_params, int32_t max_iter, double eps, int64_t chunk_bytes, double* d_warp, double* d_rho, int32_t* d_iters,
	int32_t* d_status)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, d_template && d_frames && d_warp && d_rho && d_iters && d_status, "tp_motion_ecc: null pointer");
	TP_REQUIRE(ctx, n_params == 2 || n_params == 3 || n_params == 6, "tp_motion_ecc: n_params must be 2 (translation), 3 (euclidian) or 6 (affine)");
	TP_REQUIRE(ctx, n_frames >= 0 && frame_rows >= 3 && frame_cols >= 3 && frame_rows <= 65535 && frame_cols <= 65535
		&& frame_stride >= (int64_t)frame_rows * frame_cols, "tp_motion_ecc: bad frame geometry");
	TP_REQUIRE(ctx, max_iter >= 0 && eps >= 0.0 && chunk_bytes >= 0, "tp_motion_ecc: bad termination criteria");
	if (n_frames == 0) return TP_OK;
	const int64_t n_pix = (int64_t)frame_rows * frame_cols;
	const int64_t frame_bytes = n_pix * (int64_t)sizeof(float);
	if (chunk_bytes == 0) chunk_bytes = (int64_t)2 << 30;
	const int32_t chunk = (int32_t)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n_frames, chunk_bytes / frame_bytes, 65535}));
	const int tiles = ((frame_cols + kIterTileC - 1) / kIterTileC) * ((frame_rows + kIterTileR - 1) / kIterTileR);
	const int K = n_params == 2 ? Acc<2>::K : (n_params == 3 ? Acc<3>::K : Acc<6>::K);
	void *tmpl = nullptr, *blur = nullptr, *partial = nullptr, *list = nullptr, *last = nullptr;
	int rc = TP_OK;
	auto alloc = [&](void** p, uint64_t bytes) { if (rc == TP_OK) rc = tp_malloc(ctx, bytes, p); };
	alloc(&tmpl, (uint64_t)frame_bytes);
	alloc(&blur, (uint64_t)chunk * frame_bytes);
	alloc(&partial, (uint64_t)chunk * tiles * K * sizeof(double));
	alloc(&list, (uint64_t)chunk * sizeof(int32_t));
	alloc(&last, (uint64_t)n_frames * sizeof(double));
	if (rc == TP_OK) {
		TP_LAUNCH(ctx, TPK_MOTION_INIT, tp_motion_init_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, (int)n_frames, d_warp, d_rho,
			(double*)last, d_iters, d_status, eps, max_iter);
		const dim3 tgrid((unsigned)((frame_cols + kPrepTileC - 1) / kPrepTileC), (unsigned)((frame_rows + kPrepTileR - 1) / kPrepTileR), 1);
		TP_LAUNCH(ctx, TPK_MOTION_BLUR, tp_motion_blur_kernel, tgrid, dim3(kThreads), 0, d_template, nullptr, n_pix, (int)frame_rows, (int)frame_cols,
			(float*)tmpl);
		hipError_t e = hipGetLastError();
		if (e != hipSuccess) rc = ctx->fail(TP_ERR_HIP, "tp_motion_blur_kernel", e);
	}
	if (rc == TP_OK) {
		if (n_params == 2)
			rc = ecc_chunks<2>(ctx, (const float*)tmpl, d_frames, n_frames, frame_rows, frame_cols, frame_stride, max_iter, eps, chunk, (float*)blur,
				(double*)partial, (int32_t*)list, d_warp, d_rho, (double*)last, d_iters, d_status);
		else if (n_params == 3)
			rc = ecc_chunks<3>(ctx, (const float*)tmpl, d_frames, n_frames, frame_rows, frame_cols, frame_stride, max_iter, eps, chunk, (float*)blur,
				(double*)partial, (int32_t*)list, d_warp, d_rho, (double*)last, d_iters, d_status);
		else
			rc = ecc_chunks<6>(ctx, (const float*)tmpl, d_frames, n_frames, frame_rows, frame_cols, frame_stride, max_iter, eps, chunk, (float*)blur,
				(double*)partial, (int32_t*)list, d_warp, d_rho, (double*)last, d_iters, d_status);
	}
	for (void* p : {tmpl, blur, partial, list, last}) if (p) tp_free(ctx, p);
	return rc;
	TP_API_END(ctx)
}

extern "C" int tp_motion_interpolate(tp_ctx* ctx, int32_t warpmode, int32_t n_series, const double* d_times, const double* d_kernels,
	const double* d_fill_first, const double* d_fill_last, int32_t n_times, const double* d_query, double* d_out)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const int P = warp_params(warpmode);
	TP_REQUIRE(ctx, P >= 0, "tp_motion_interpolate: warpmode must be TP_MOTION_UNCHANGED, _TRANSLATION, _EUCLIDIAN or _AFFINE");
	TP_REQUIRE(ctx, n_series >= 2 && n_times >= 0, "tp_motion_interpolate: a series of at least two kernels and n_times >= 0 expected");
	if (n_times == 0 || P == 0) return TP_OK;
	TP_REQUIRE(ctx, d_times && d_kernels && d_fill_first && d_fill_last && d_query && d_out, "tp_motion_interpolate: null pointer");
	return launch_interp(ctx, warpmode, n_series, d_times, d_kernels, d_fill_first, d_fill_last, n_times, d_query, d_out, nullptr);
	TP_API_END(ctx)
}

extern "C" int tp_motion_star_positions(tp_ctx* ctx, int32_t warpmode, int32_t n_series, const double* d_times, const double* d_kernels,
	const double* d_fill_first, const double* d_fill_last, int32_t n_times, const double* d_query, int64_t n, const double* d_xy, int32_t single,
	const float* d_base_col, const float* d_base_row, const int64_t* d_out_index, int64_t n_out, double* d_pos_col, double* d_pos_row,
	int64_t pos_pitch, double* d_jitter)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const int P = warp_params(warpmode);
	TP_REQUIRE(ctx, P >= 0, "tp_motion_star_positions: warpmode must be TP_MOTION_UNCHANGED, _TRANSLATION, _EUCLIDIAN or _AFFINE");
	TP_REQUIRE(ctx, n_series >= 2 && n_times >= 0 && n >= 0 && n_out >= 0 && pos_pitch >= n_times && (single == 0 || single == 1),
		"tp_motion_star_positions: bad arguments (a series of at least two kernels, sizes >= 0, pos_pitch >= n_times expected)");
	if (n_times == 0 || n == 0) return TP_OK;
	TP_REQUIRE(ctx, d_times && d_query && d_xy && (P == 0 || (d_kernels && d_fill_first && d_fill_last))
		&& (n_out == 0 || (d_base_col && d_base_row && d_out_index && d_pos_col && d_pos_row)), "tp_motion_star_positions: null pointer");
	const int tiles = (n_times + kThreads - 1) / kThreads;
	const int64_t blocks = ((n + kPosStars - 1) / kPosStars) * tiles;
	TP_REQUIRE(ctx, blocks <= 0x7fffffff, "tp_motion_star_positions: too many positions times cadences for one launch");
	double* mats = nullptr;
	int rc = tp_malloc(ctx, (uint64_t)n_times * 6 * sizeof(double), (void**)&mats);
	if (rc != TP_OK) return rc;
	rc = launch_interp(ctx, warpmode, n_series, d_times, d_kernels, d_fill_first, d_fill_last, n_times, d_query, nullptr, mats);
	if (rc == TP_OK) {
		StarArgs A{(int)warpmode, (int)single, (int)n_times, mats, n, d_xy, d_base_col, d_base_row, d_out_index, n_out, d_pos_col, d_pos_row, pos_pitch,
			d_jitter, tiles};
		TP_LAUNCH(ctx, TPK_MOTION_POSITIONS, tp_motion_positions_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, A);
		hipError_t e = hipGetLastError();
		if (e != hipSuccess) rc = ctx->fail(TP_ERR_HIP, "tp_motion_positions_kernel", e);
	}
	tp_free(ctx, mats);
	return rc;
	TP_API_END(ctx)
}
