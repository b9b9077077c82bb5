// halo.hip -- Halo photometry (photometry/halo/halo_photometry.py:86-265) on the device: the TV-min pixel weights of Pope et al.
// (2016, 2019) for a batch of problems (one problem = one light-curve segment of one target).
//
// Problem i: P[t][p] float32, ncad rows of `pitch` = round_up(npix, 4) floats (zero padded) from d_P + p_offset[i]; fit[t] marks
// the fitted cadences F (in time order).  Weights w = softmax(theta), l_t = sum_p w_p P[t][p] (float64),
// f = sum_j |l_F[j+1] - l_F[j]| / median(l_F) (numpy's median), minimised over theta by L-BFGS (two-loop recursion, history H,
// H0 = gamma I from the newest pair, first direction -g / |g|_2) with a backtracking Armijo line search (alpha = 1, c1 = 1e-4,
// halving, 20 trials) from theta = 0; stop at maxiter iterations, f_k - f_k+1 <= ftol max(|f_k|, |f_k+1|, 1) or |grad|_inf <= gtol.
// The definition the device is held to is tests/halo_common.py ("Halo").
//
// One step = one evaluation of every active problem:
//   forward  (problem, cadence tile): l of the tile from w, dwordx4 rows, float64 accumulation;
//   stat     (one block per problem): the exact median of l_F (radix select on the order-preserving 64-bit key, 256-bin LDS
//            histogram per pass), the TV sum and the sign terms s_t, the Armijo decision and, on rejection, the next trial's w;
//   backward (problem, cadence tile), accepted points only: the tile's partial sum_t P[t][p] s_t;
//   finish   (one block per problem), accepted points only: the tile partials summed in a fixed order, the median term, the
//            softmax chain rule, the history update, the stopping tests, the two-loop recursion and the next trial's w.
// The host loop polls the problem states and relaunches over the problems still active (as csrc/motion.hip).  No float atomics:
// every reduction has a fixed order, so a problem gives the same bits alone as inside a batch.
#include "common.h"
#include <cmath>
#include <vector>
#include <algorithm>

namespace {

constexpr int kTile = 64;            // cadences per forward / backward block
constexpr int kThreads = 256;        // forward / backward / finish / init / output blocks
constexpr int kStatThreads = 1024;   // stat block: one per problem
constexpr int kKR = 20;              // keys cached in registers per stat thread (20 480 fitted cadences; the rest are re-read)
constexpr int kMaxPitch = 4096;      // pixels per problem
constexpr int kMaxChunks = kMaxPitch / 4 / kThreads;
constexpr int kMaxHistory = 16;
constexpr int kMaxTrials = 20;
constexpr double kC1 = 1e-4;
constexpr double kPairCurv = 1e-10;

enum { ST_ACTIVE = 0, ST_CONVERGED = 1, ST_CAP = 2, ST_LINESEARCH = 3, ST_DEGENERATE = 4 };

struct HaloProb {
	int64_t p_off;      // P element offset (multiple of 4)
	int64_t c_off;      // cadence offset: fit, l, fidx, sgn
	int64_t w_off;      // offset of the pitch-padded pixel arrays (theta, g, d, w, q)
	int64_t o_off;      // offset of the unpadded pixel outputs (d_w, theta in, gradient out)
	int64_t h_off;      // offset of the history S / Y: pair k at h_off + k * pitch
	int64_t part_off;   // offset of the backward partials [ntiles][pitch]
	int32_t npix, pitch, ncad, ntiles;
};

struct HaloState {
	double f, f_prev, alpha, gtd, m;
	int32_t status, iters, trials, need_grad, initial, n_pairs, newest, nf, tmed0, tmed1;
};

struct HaloArgs {
	const HaloProb* prob;
	HaloState* state;
	const float* P;
	const uint8_t* fit;
	double* l;
	int32_t* fidx;
	float* sgn;
	double *theta, *g, *d, *w, *q;
	double *S, *Y;
	double* partial;
	double* pairs;       // [problem][kMaxHistory][2]: s.y and y.y of the stored pairs
	int32_t maxiter, history;
	double ftol, gtol;
	int32_t objective;   // 1: one evaluation (tp_halo_objective), the gradient goes to grad_out
	double* grad_out;
};

__device__ inline double wave_sum(double v) {
	for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}
__device__ inline double wave_max(double v) {
	for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
	return v;
}

// fixed-order block reductions (every thread gets the result)
template <int NT> __device__ double block_sum(double v, double* red) {
	v = wave_sum(v);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	double s = red[0];
	for (int k = 1; k < NT / 64; k++) s += red[k];
	__syncthreads();
	return s;
}
template <int NT> __device__ double block_max(double v, double* red) {
	v = wave_max(v);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	double s = red[0];
	for (int k = 1; k < NT / 64; k++) s = fmax(s, red[k]);
	__syncthreads();
	return s;
}

// w = softmax(theta + alpha d) (d null: softmax(theta)); zero in the padding.  Each thread touches only its own entries of w.
template <int NT> __device__ void softmax_into(const double* th, const double* d, double alpha, int npix, int pitch, double* w, double* red) {
	double mx = -INFINITY;
	for (int p = threadIdx.x; p < npix; p += NT) mx = fmax(mx, d ? th[p] + alpha * d[p] : th[p]);
	mx = block_max<NT>(mx, red);
	double s = 0.0;
	for (int p = threadIdx.x; p < npix; p += NT) {
		const double e = exp((d ? th[p] + alpha * d[p] : th[p]) - mx);
		w[p] = e;
		s += e;
	}
	s = block_sum<NT>(s, red);
	for (int p = threadIdx.x; p < pitch; p += NT) w[p] = p < npix ? w[p] / s : 0.0;
}

__device__ inline uint64_t okey(double v) {
	const uint64_t u = (uint64_t)__double_as_longlong(v);
	return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double from_key(uint64_t k) {
	return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// ---- init: fitted-cadence list, sign terms zeroed, theta, w, state ---------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tp_halo_init_kernel(HaloArgs a, const double* theta_in)
{
	const int pi = blockIdx.x;
	const HaloProb pr = a.prob[pi];
	__shared__ double red[kThreads / 64];
	__shared__ int wcount[kThreads / 64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int base = 0;
	for (int c0 = 0; c0 < pr.ncad; c0 += kThreads) {
		const int t = c0 + threadIdx.x;
		const bool flag = t < pr.ncad && a.fit[pr.c_off + t] != 0;
		if (t < pr.ncad) a.sgn[pr.c_off + t] = 0.0f;
		const unsigned long long b = __ballot(flag);
		if (lane == 0) wcount[wave] = __popcll(b);
		__syncthreads();
		int before = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
		for (int k = 0; k < kThreads / 64; k++) {
			if (k < wave) before += wcount[k];
			total += wcount[k];
		}
		if (flag) a.fidx[pr.c_off + base + before] = t;
		base += total;
		__syncthreads();
	}
	double* th = a.theta + pr.w_off;
	for (int p = threadIdx.x; p < pr.pitch; p += kThreads) {
		th[p] = (theta_in && p < pr.npix) ? theta_in[pr.o_off + p] : 0.0;
		a.d[pr.w_off + p] = 0.0;
		a.g[pr.w_off + p] = 0.0;
	}
	softmax_into<kThreads>(th, nullptr, 0.0, pr.npix, pr.pitch, a.w + pr.w_off, red);
	if (threadIdx.x == 0) {
		HaloState& s = a.state[pi];
		s.f = s.f_prev = s.gtd = s.m = 0.0;
		s.alpha = 1.0;
		s.iters = s.trials = s.need_grad = s.n_pairs = 0;
		s.newest = -1;
		s.initial = 1;
		s.nf = base;
		s.tmed0 = s.tmed1 = 0;
		s.status = base < 3 ? ST_DEGENERATE : ST_ACTIVE;
	}
}

// ---- forward: l of a cadence tile --------------------------------------------------------------------------------------------
// block = 4 waves, one row per wave at a time; list2: (problem, tile) pairs
__global__ __launch_bounds__(kThreads) void tp_halo_forward_kernel(HaloArgs a, const int32_t* __restrict__ list2, int32_t all)
{
	extern __shared__ double sw[];
	const int pi = list2[2 * blockIdx.x], tile = list2[2 * blockIdx.x + 1];
	if (!all && a.state[pi].status != ST_ACTIVE) return;
	const HaloProb pr = a.prob[pi];
	const double* w = a.w + pr.w_off;
	for (int p = threadIdx.x; p < pr.pitch; p += kThreads) sw[p] = w[p];
	__syncthreads();
	const int nch = pr.pitch >> 2;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int t1 = min((tile + 1) * kTile, pr.ncad);
	for (int t = tile * kTile + wave; t < t1; t += kThreads / 64) {
		const float4* row = reinterpret_cast<const float4*>(a.P + pr.p_off + (int64_t)t * pr.pitch);
		double acc = 0.0;
		for (int c = lane; c < nch; c += 64) {
			const float4 v = row[c];
			const double* ww = sw + 4 * c;
			acc += ((ww[0] * (double)v.x + ww[1] * (double)v.y) + (ww[2] * (double)v.z + ww[3] * (double)v.w));
		}
		acc = wave_sum(acc);
		if (lane == 0) a.l[pr.c_off + t] = acc;
	}
}

// ---- stat: median, TV, sign terms, Armijo decision -------------------------------------------------------------------------
struct Select {
	uint64_t key;
	int rank;   // how many equal keys precede the selected one in time order (its occurrence index)
};

__device__ Select radix_select(const uint64_t (&kc)[kKR], const double* l, const int32_t* fidx, int nf, int k, int* hist, int* sh) {
	uint64_t prefix = 0, mask = 0;
	int krem = k;
	for (int shift = 56; shift >= 0; shift -= 8) {
		for (int b = threadIdx.x; b < 256; b += kStatThreads) hist[b] = 0;
		__syncthreads();
#pragma unroll
		for (int r = 0; r < kKR; r++) {
			const int j = r * kStatThreads + (int)threadIdx.x;
			if (j < nf && (kc[r] & mask) == prefix) atomicAdd(&hist[(kc[r] >> shift) & 255], 1);
		}
		for (int j = kKR * kStatThreads + (int)threadIdx.x; j < nf; j += kStatThreads) {
			const uint64_t key = okey(l[fidx[j]]);
			if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1);
		}
		__syncthreads();
		if (threadIdx.x < 64) {
			const int lane = threadIdx.x;
			const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
			const int s = c0 + c1 + c2 + c3;
			int inc = s;
			for (int o = 1; o < 64; o <<= 1) {
				const int v = __shfl_up(inc, o, 64);
				if (lane >= o) inc += v;
			}
			const int exc = inc - s;
			if (exc <= krem && krem < inc) {
				int b = 4 * lane, cum = exc;
				if (krem >= cum + c0) {
					cum += c0; b++;
					if (krem >= cum + c1) {
						cum += c1; b++;
						if (krem >= cum + c2) { cum += c2; b++; }
					}
				}
				sh[0] = b;
				sh[1] = krem - cum;
			}
		}
		__syncthreads();
		prefix |= (uint64_t)sh[0] << shift;
		krem = sh[1];
		mask |= (uint64_t)255 << shift;
		__syncthreads();
	}
	return Select{prefix, krem};
}

// the cadence (problem-local index) of the rank-th occurrence, in time order, of the key among the fitted l
__device__ int find_occurrence(const double* l, const int32_t* fidx, int nf, uint64_t key, int rank, int* wcount, int* sh) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (threadIdx.x == 0) sh[2] = -1;
	__syncthreads();
	for (int base = 0; base < nf; base += kStatThreads) {
		const int j = base + (int)threadIdx.x;
		const bool match = j < nf && okey(l[fidx[j]]) == key;
		const unsigned long long b = __ballot(match);
		if (lane == 0) wcount[wave] = __popcll(b);
		__syncthreads();
		int before = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
		for (int k = 0; k < kStatThreads / 64; k++) {
			if (k < wave) before += wcount[k];
			total += wcount[k];
		}
		if (match && before == rank) sh[2] = fidx[j];
		__syncthreads();
		if (sh[2] >= 0) break;
		rank -= total;
	}
	const int r = sh[2];
	__syncthreads();
	return r;
}

__global__ __launch_bounds__(kStatThreads) void tp_halo_stat_kernel(HaloArgs a, const int32_t* __restrict__ plist)
{
	const int pi = plist[blockIdx.x];
	const HaloState st = a.state[pi];
	if (st.status != ST_ACTIVE) return;
	const HaloProb pr = a.prob[pi];
	__shared__ int hist[256];
	__shared__ int sh[4];
	__shared__ int wcount[kStatThreads / 64];
	__shared__ double red[kStatThreads / 64];
	const int nf = st.nf;
	const double* l = a.l + pr.c_off;
	const int32_t* fidx = a.fidx + pr.c_off;
	float* sgn = a.sgn + pr.c_off;
	uint64_t kc[kKR];
#pragma unroll
	for (int r = 0; r < kKR; r++) {
		const int j = r * kStatThreads + (int)threadIdx.x;
		kc[r] = j < nf ? okey(l[fidx[j]]) : 0;
	}
	// TV and the sign terms s_t = sign(l_j - l_j-1) - sign(l_j+1 - l_j) (sign(0) = 0, the ends have one neighbour)
	double tv = 0.0;
	for (int j = threadIdx.x; j < nf; j += kStatThreads) {
		const double v = l[fidx[j]];
		const double dp = j > 0 ? v - l[fidx[j - 1]] : 0.0;
		const double dn = j + 1 < nf ? l[fidx[j + 1]] - v : 0.0;
		sgn[fidx[j]] = (float)(((dp > 0.0) - (dp < 0.0)) - ((dn > 0.0) - (dn < 0.0)));
		tv += fabs(dn);
	}
	tv = block_sum<kStatThreads>(tv, red);
	const int k1 = (nf - 1) / 2, k2 = nf / 2;
	const Select s1 = radix_select(kc, l, fidx, nf, k1, hist, sh);
	Select s2 = s1;
	if (k2 != k1) s2 = radix_select(kc, l, fidx, nf, k2, hist, sh);
	const double m = k2 != k1 ? (from_key(s1.key) + from_key(s2.key)) / 2.0 : from_key(s1.key);
	const bool valid = m > 0.0 && isfinite(m);
	const double ft = valid ? tv / m : INFINITY;
	HaloState& so = a.state[pi];
	// decision (uniform over the block)
	bool accept;
	if (st.initial) {
		accept = valid;
		if (!valid && threadIdx.x == 0) so.status = ST_DEGENERATE;
	} else {
		accept = valid && ft <= st.f + kC1 * st.alpha * st.gtd;
	}
	if (accept) {
		const int t0 = find_occurrence(l, fidx, nf, s1.key, s1.rank, wcount, sh);
		const int t1 = k2 != k1 ? find_occurrence(l, fidx, nf, s2.key, s2.rank, wcount, sh) : t0;
		if (threadIdx.x == 0) {
			if (!st.initial) {
				so.f_prev = st.f;
				so.iters = st.iters + 1;
			}
			so.f = ft;
			so.m = m;
			so.tmed0 = t0;
			so.tmed1 = t1;
			so.need_grad = 1;
		}
	} else if (!st.initial) {
		const int trials = st.trials + 1;
		if (trials >= kMaxTrials) {
			if (threadIdx.x == 0) {
				so.trials = trials;
				so.need_grad = 0;
				so.status = ST_LINESEARCH;
			}
		} else {
			const double alpha = st.alpha * 0.5;
			softmax_into<kStatThreads>(a.theta + pr.w_off, a.d + pr.w_off, alpha, pr.npix, pr.pitch, a.w + pr.w_off, red);
			if (threadIdx.x == 0) {
				so.trials = trials;
				so.alpha = alpha;
				so.need_grad = 0;
			}
		}
	}
}

// ---- backward: partial sum_t P[t][p] s_t of a cadence tile ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tp_halo_backward_kernel(HaloArgs a, const int32_t* __restrict__ list2)
{
	const int pi = list2[2 * blockIdx.x], tile = list2[2 * blockIdx.x + 1];
	{
		const HaloState& st = a.state[pi];
		if (st.status != ST_ACTIVE || !st.need_grad) return;
	}
	const HaloProb pr = a.prob[pi];
	const int nch = pr.pitch >> 2;
	double acc[kMaxChunks][4];
#pragma unroll
	for (int k = 0; k < kMaxChunks; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0;
	const int t1 = min((tile + 1) * kTile, pr.ncad);
	const float* sgn = a.sgn + pr.c_off;
	for (int t = tile * kTile; t < t1; t++) {
		const float s = sgn[t];
		if (s == 0.0f) continue;   // uniform: every thread reads the same row
		const double sd = (double)s;
		const float4* row = reinterpret_cast<const float4*>(a.P + pr.p_off + (int64_t)t * pr.pitch);
#pragma unroll
		for (int k = 0; k < kMaxChunks; k++) {
			const int c = (int)threadIdx.x + k * kThreads;
			if (c < nch) {
				const float4 v = row[c];
				acc[k][0] += sd * (double)v.x;
				acc[k][1] += sd * (double)v.y;
				acc[k][2] += sd * (double)v.z;
				acc[k][3] += sd * (double)v.w;
			}
		}
	}
	double* out = a.partial + pr.part_off + (int64_t)tile * pr.pitch;
#pragma unroll
	for (int k = 0; k < kMaxChunks; k++) {
		const int c = (int)threadIdx.x + k * kThreads;
		if (c < nch) {
			out[4 * c] = acc[k][0];
			out[4 * c + 1] = acc[k][1];
			out[4 * c + 2] = acc[k][2];
			out[4 * c + 3] = acc[k][3];
		}
	}
}

// ---- finish: gradient, history, stopping tests, next direction -------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tp_halo_finish_kernel(HaloArgs a, const int32_t* __restrict__ plist)
{
	const int pi = plist[blockIdx.x];
	const HaloState st = a.state[pi];
	if (st.status != ST_ACTIVE || !st.need_grad) return;
	const HaloProb pr = a.prob[pi];
	__shared__ double red[kThreads / 64];
	__shared__ double sa[kMaxHistory], ssy[kMaxHistory], syy[kMaxHistory];
	const int npix = pr.npix, pitch = pr.pitch, H = a.history;
	double* pairs = a.pairs ? a.pairs + (int64_t)pi * kMaxHistory * 2 : nullptr;
	if (pairs && threadIdx.x < H) {
		ssy[threadIdx.x] = pairs[2 * threadIdx.x];
		syy[threadIdx.x] = pairs[2 * threadIdx.x + 1];
	}
	const double m = st.m, f = st.f, fm = f / m;
	const float* r0 = a.P + pr.p_off + (int64_t)st.tmed0 * pitch;
	const float* r1 = a.P + pr.p_off + (int64_t)st.tmed1 * pitch;
	const double* part = a.partial + pr.part_off;
	double* th = a.theta + pr.w_off;
	double* g = a.g + pr.w_off;
	double* d = a.d + pr.w_off;
	double* w = a.w + pr.w_off;
	double* q = a.q + pr.w_off;
	// gradient with respect to w, then through the softmax: q = w (g - w.g)
	double acc = 0.0;
	for (int p = threadIdx.x; p < npix; p += kThreads) {
		// the tile partials in a fixed order: four interleaved chains (tiles t = k mod 4), then (0 + 1) + (2 + 3)
		double G0 = 0.0, G1 = 0.0, G2 = 0.0, G3 = 0.0;
		int t = 0;
		for (; t + 4 <= pr.ntiles; t += 4) {
			G0 += part[(int64_t)t * pitch + p];
			G1 += part[(int64_t)(t + 1) * pitch + p];
			G2 += part[(int64_t)(t + 2) * pitch + p];
			G3 += part[(int64_t)(t + 3) * pitch + p];
		}
		if (t < pr.ntiles) G0 += part[(int64_t)t * pitch + p];
		if (t + 1 < pr.ntiles) G1 += part[(int64_t)(t + 1) * pitch + p];
		if (t + 2 < pr.ntiles) G2 += part[(int64_t)(t + 2) * pitch + p];
		const double G = (G0 + G1) + (G2 + G3);
		const double pm = st.tmed0 == st.tmed1 ? (double)r0[p] : ((double)r0[p] + (double)r1[p]) * 0.5;
		const double gw = G / m - fm * pm;
		q[p] = gw;
		acc += w[p] * gw;
	}
	const double wg = block_sum<kThreads>(acc, red);
	double gmax = 0.0;
	for (int p = threadIdx.x; p < npix; p += kThreads) {
		const double gt = w[p] * (q[p] - wg);
		q[p] = gt;
		gmax = fmax(gmax, fabs(gt));
	}
	gmax = block_max<kThreads>(gmax, red);
	HaloState& so = a.state[pi];
	int status = ST_ACTIVE;
	int n_pairs = st.n_pairs, newest = st.newest;
	if (st.initial) {
		if (a.objective) {
			for (int p = threadIdx.x; p < npix; p += kThreads) a.grad_out[pr.o_off + p] = q[p];
			if (threadIdx.x == 0) {
				so.status = ST_CONVERGED;
				so.need_grad = 0;
				so.initial = 0;
			}
			return;
		}
		for (int p = threadIdx.x; p < npix; p += kThreads) g[p] = q[p];
		if (gmax <= a.gtol) status = ST_CONVERGED;
		else if (a.maxiter <= 0) status = ST_CAP;
	} else {
		// s = theta_new - theta, y = grad_new - grad; the pair is kept if s.y > 1e-10 y.y
		double sy = 0.0, yy = 0.0;
		for (int p = threadIdx.x; p < npix; p += kThreads) {
			const double tn = th[p] + st.alpha * d[p];
			const double s = tn - th[p], y = q[p] - g[p];
			sy += s * y;
			yy += y * y;
		}
		sy = block_sum<kThreads>(sy, red);
		yy = block_sum<kThreads>(yy, red);
		const bool keep = sy > kPairCurv * yy;
		const int slot = (newest + 1) % H;
		double* Sk = a.S + pr.h_off + (int64_t)slot * pitch;
		double* Yk = a.Y + pr.h_off + (int64_t)slot * pitch;
		for (int p = threadIdx.x; p < npix; p += kThreads) {
			const double tn = th[p] + st.alpha * d[p];
			if (keep) {
				Sk[p] = tn - th[p];
				Yk[p] = q[p] - g[p];
			}
			th[p] = tn;
			g[p] = q[p];
		}
		if (keep) {
			newest = slot;
			n_pairs = min(n_pairs + 1, H);
			if (threadIdx.x == 0) {
				ssy[slot] = sy;
				syy[slot] = yy;
				pairs[2 * slot] = sy;
				pairs[2 * slot + 1] = yy;
			}
		}
		if (st.f_prev - f <= a.ftol * fmax(fmax(fabs(st.f_prev), fabs(f)), 1.0)) status = ST_CONVERGED;
		else if (gmax <= a.gtol) status = ST_CONVERGED;
		else if (st.iters >= a.maxiter) status = ST_CAP;
	}
	if (status != ST_ACTIVE) {
		__syncthreads();
		if (threadIdx.x == 0) {
			so.status = status;
			so.need_grad = 0;
			so.initial = 0;
			so.n_pairs = n_pairs;
			so.newest = newest;
		}
		return;
	}
	__syncthreads();   // the scalars of the new pair visible to every thread
	// direction: the two-loop recursion over the pairs (oldest .. newest), or -g / |g|_2
	double gtd = 0.0;
	if (n_pairs > 0) {
		for (int p = threadIdx.x; p < npix; p += kThreads) d[p] = g[p];
		for (int i = n_pairs - 1; i >= 0; i--) {
			const int k = (newest - (n_pairs - 1 - i) + H) % H;
			const double* Sk = a.S + pr.h_off + (int64_t)k * pitch;
			const double* Yk = a.Y + pr.h_off + (int64_t)k * pitch;
			double v = 0.0;
			for (int p = threadIdx.x; p < npix; p += kThreads) v += Sk[p] * d[p];
			const double ai = (1.0 / ssy[k]) * block_sum<kThreads>(v, red);
			if (threadIdx.x == 0) sa[i] = ai;
			for (int p = threadIdx.x; p < npix; p += kThreads) d[p] -= ai * Yk[p];
		}
		const double gamma = ssy[newest] / syy[newest];
		for (int p = threadIdx.x; p < npix; p += kThreads) d[p] = gamma * d[p];
		__syncthreads();
		for (int i = 0; i < n_pairs; i++) {
			const int k = (newest - (n_pairs - 1 - i) + H) % H;
			const double* Sk = a.S + pr.h_off + (int64_t)k * pitch;
			const double* Yk = a.Y + pr.h_off + (int64_t)k * pitch;
			double v = 0.0;
			for (int p = threadIdx.x; p < npix; p += kThreads) v += Yk[p] * d[p];
			const double b = (1.0 / ssy[k]) * block_sum<kThreads>(v, red);
			const double ai = sa[i];
			for (int p = threadIdx.x; p < npix; p += kThreads) d[p] += Sk[p] * (ai - b);
		}
		double v = 0.0;
		for (int p = threadIdx.x; p < npix; p += kThreads) {
			d[p] = -d[p];
			v += g[p] * d[p];
		}
		gtd = block_sum<kThreads>(v, red);
		if (!(gtd < 0.0)) n_pairs = 0;   // not a descent direction: the history is dropped
	}
	if (n_pairs == 0) {
		double v = 0.0;
		for (int p = threadIdx.x; p < npix; p += kThreads) v += g[p] * g[p];
		const double nrm = sqrt(block_sum<kThreads>(v, red));
		v = 0.0;
		for (int p = threadIdx.x; p < npix; p += kThreads) {
			d[p] = -g[p] / nrm;
			v += g[p] * d[p];
		}
		gtd = block_sum<kThreads>(v, red);
	}
	softmax_into<kThreads>(th, d, 1.0, npix, pitch, w, red);
	if (threadIdx.x == 0) {
		so.alpha = 1.0;
		so.trials = 0;
		so.gtd = gtd;
		so.need_grad = 0;
		so.initial = 0;
		so.n_pairs = n_pairs;
		so.newest = newest;
	}
}

// ---- output: w = softmax(theta), f, iterations, status ---------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tp_halo_output_kernel(HaloArgs a, double* d_w, double* d_f, int32_t* d_iters, int32_t* d_status)
{
	const int pi = blockIdx.x;
	const HaloProb pr = a.prob[pi];
	const HaloState st = a.state[pi];
	__shared__ double red[kThreads / 64];
	double* w = a.w + pr.w_off;
	softmax_into<kThreads>(a.theta + pr.w_off, nullptr, 0.0, pr.npix, pr.pitch, w, red);
	const bool degenerate = st.status == ST_DEGENERATE;
	if (d_w)
		for (int p = threadIdx.x; p < pr.npix; p += kThreads) d_w[pr.o_off + p] = w[p];
	if (a.objective && degenerate)
		for (int p = threadIdx.x; p < pr.npix; p += kThreads) a.grad_out[pr.o_off + p] = NAN;
	if (threadIdx.x == 0) {
		if (d_f) d_f[pi] = degenerate ? NAN : st.f;
		if (d_iters) d_iters[pi] = st.iters;
		if (d_status) d_status[pi] = st.status;
	}
}

int halo_run(tp_ctx* ctx, int32_t n, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad, const float* d_P,
	const uint8_t* d_fit, const double* d_theta, int32_t maxiter, int32_t history, double ftol, double gtol, int objective,
	double* d_w, double* d_l, double* d_f, int32_t* d_iters, int32_t* d_status, double* d_grad)
{
	std::vector<HaloProb> prob(n);
	int64_t c_tot = 0, w_tot = 0, o_tot = 0, part_tot = 0, tiles_tot = 0;
	int32_t max_pitch = 4;
	for (int i = 0; i < n; i++) {
		HaloProb& p = prob[i];
		p.npix = h_npix[i];
		p.pitch = (h_npix[i] + 3) & ~3;
		p.ncad = h_ncad[i];
		p.ntiles = (h_ncad[i] + kTile - 1) / kTile;
		p.p_off = h_p_offset[i];
		p.c_off = c_tot;
		p.w_off = w_tot;
		p.o_off = o_tot;
		p.h_off = w_tot * history;
		p.part_off = part_tot;
		c_tot += p.ncad;
		w_tot += p.pitch;
		o_tot += p.npix;
		part_tot += (int64_t)p.ntiles * p.pitch;
		tiles_tot += p.ntiles;
		max_pitch = std::max(max_pitch, p.pitch);
	}
	TP_REQUIRE(ctx, tiles_tot < (int64_t)1 << 30 && c_tot < (int64_t)1 << 31, "tp_halo: too many cadences");
	void *dprob = nullptr, *dstate = nullptr, *dl = nullptr, *dfidx = nullptr, *dsgn = nullptr, *dpix = nullptr, *dhist = nullptr,
		*dpart = nullptr, *dlist2 = nullptr, *dplist = nullptr, *dpairs = nullptr;
	int rc = TP_OK;
	auto alloc = [&](void** ptr, uint64_t bytes) { if (rc == TP_OK) rc = tp_malloc(ctx, std::max<uint64_t>(bytes, 16), ptr); };
	alloc(&dprob, (uint64_t)n * sizeof(HaloProb));
	alloc(&dstate, (uint64_t)n * sizeof(HaloState));
	if (!d_l) alloc(&dl, (uint64_t)c_tot * sizeof(double));
	alloc(&dfidx, (uint64_t)c_tot * sizeof(int32_t));
	alloc(&dsgn, (uint64_t)c_tot * sizeof(float));
	alloc(&dpix, (uint64_t)w_tot * 5 * sizeof(double));
	if (!objective) alloc(&dhist, (uint64_t)w_tot * history * 2 * sizeof(double));
	if (!objective) alloc(&dpairs, (uint64_t)n * kMaxHistory * 2 * sizeof(double));
	alloc(&dpart, (uint64_t)part_tot * sizeof(double));
	alloc(&dlist2, (uint64_t)tiles_tot * 2 * sizeof(int32_t));
	alloc(&dplist, (uint64_t)n * sizeof(int32_t));
	if (rc == TP_OK) {
		HaloArgs a{};
		a.prob = (const HaloProb*)dprob;
		a.state = (HaloState*)dstate;
		a.P = d_P;
		a.fit = d_fit;
		a.l = d_l ? d_l : (double*)dl;
		a.fidx = (int32_t*)dfidx;
		a.sgn = (float*)dsgn;
		double* pix = (double*)dpix;
		a.theta = pix; a.g = pix + w_tot; a.d = pix + 2 * w_tot; a.w = pix + 3 * w_tot; a.q = pix + 4 * w_tot;
		a.S = dhist ? (double*)dhist : nullptr;
		a.Y = dhist ? (double*)dhist + w_tot * history : nullptr;
		a.partial = (double*)dpart;
		a.pairs = (double*)dpairs;
		a.maxiter = maxiter;
		a.history = history;
		a.ftol = ftol;
		a.gtol = gtol;
		a.objective = objective;
		a.grad_out = d_grad;
		const size_t lds = (size_t)max_pitch * sizeof(double);
		// the problem table, then the full launch lists
		std::vector<int32_t> list2, plist;
		auto build_lists = [&](const std::vector<int32_t>* st) {
			list2.clear();
			plist.clear();
			for (int i = 0; i < n; i++) {
				if (st && (*st)[i] != ST_ACTIVE) continue;
				plist.push_back(i);
				for (int t = 0; t < prob[i].ntiles; t++) { list2.push_back(i); list2.push_back(t); }
			}
		};
		auto run = [&]() -> int {
			TP_HIP(ctx, hipMemcpyAsync(dprob, prob.data(), (size_t)n * sizeof(HaloProb), hipMemcpyHostToDevice, ctx->stream));
			TP_LAUNCH(ctx, TPK_HALO_INIT, tp_halo_init_kernel, dim3((unsigned)n), dim3(kThreads), 0, a, d_theta);
			TP_LAUNCH_CHECK(ctx, "tp_halo_init_kernel");
			// the initial states (degenerate problems never start)
			std::vector<int32_t> st(n);
			std::vector<HaloState> hs(n);
			TP_HIP(ctx, hipMemcpyAsync(hs.data(), dstate, (size_t)n * sizeof(HaloState), hipMemcpyDeviceToHost, ctx->stream));
			TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
			for (int i = 0; i < n; i++) st[i] = hs[i].status;
			build_lists(&st);
			// every step moves each active problem on by one evaluation; an iteration is at most 1 + kMaxTrials of them
			const int64_t max_steps = objective ? 1 : ((int64_t)maxiter + 1) * (kMaxTrials + 1) + 1;
			int64_t done = 0;
			int32_t poll = objective ? 1 : 4;
			while (!plist.empty() && done < max_steps) {
				TP_HIP(ctx, hipMemcpyAsync(dlist2, list2.data(), list2.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
				TP_HIP(ctx, hipMemcpyAsync(dplist, plist.data(), plist.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
				const unsigned nt = (unsigned)(list2.size() / 2), np = (unsigned)plist.size();
				const int64_t steps = std::min<int64_t>(poll, max_steps - done);
				for (int64_t s = 0; s < steps; s++) {
					TP_LAUNCH(ctx, TPK_HALO_FORWARD, tp_halo_forward_kernel, dim3(nt), dim3(kThreads), lds, a, (const int32_t*)dlist2, 0);
					TP_LAUNCH(ctx, TPK_HALO_STAT, tp_halo_stat_kernel, dim3(np), dim3(kStatThreads), 0, a, (const int32_t*)dplist);
					TP_LAUNCH(ctx, TPK_HALO_BACKWARD, tp_halo_backward_kernel, dim3(nt), dim3(kThreads), 0, a, (const int32_t*)dlist2);
					TP_LAUNCH(ctx, TPK_HALO_FINISH, tp_halo_finish_kernel, dim3(np), dim3(kThreads), 0, a, (const int32_t*)dplist);
				}
				TP_LAUNCH_CHECK(ctx, "tp_halo_forward_kernel");
				done += steps;
				TP_HIP(ctx, hipMemcpyAsync(hs.data(), dstate, (size_t)n * sizeof(HaloState), hipMemcpyDeviceToHost, ctx->stream));
				TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
				for (int i = 0; i < n; i++) st[i] = hs[i].status;
				build_lists(&st);
				poll = std::min(poll * 2, 32);
			}
			TP_LAUNCH(ctx, TPK_HALO_OUTPUT, tp_halo_output_kernel, dim3((unsigned)n), dim3(kThreads), 0, a, d_w, d_f, d_iters, d_status);
			if (d_l) {
				build_lists(nullptr);
				if (!list2.empty()) {
					TP_HIP(ctx, hipMemcpyAsync(dlist2, list2.data(), list2.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
					TP_LAUNCH(ctx, TPK_HALO_FORWARD, tp_halo_forward_kernel, dim3((unsigned)(list2.size() / 2)), dim3(kThreads), lds, a,
						(const int32_t*)dlist2, 1);
				}
			}
			TP_LAUNCH_CHECK(ctx, "tp_halo_output_kernel");
			// the host vectors the asynchronous copies read must outlive them
			TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
			return TP_OK;
		};
		rc = run();
	}
	for (void* p : {dprob, dstate, dl, dfidx, dsgn, dpix, dhist, dpart, dlist2, dplist, dpairs}) if (p) tp_free(ctx, p);
	return rc;
}

int halo_check(tp_ctx* ctx, int32_t n, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad, const float* d_P, const uint8_t* d_fit)
{
	TP_REQUIRE(ctx, n >= 0 && n <= (1 << 24), "tp_halo: bad problem count");
	if (n == 0) return TP_OK;
	TP_REQUIRE(ctx, h_p_offset && h_npix && h_ncad && d_P && d_fit, "tp_halo: null pointer");
	TP_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_P) & 15u) == 0, "tp_halo: d_P must be 16-byte aligned");
	for (int i = 0; i < n; i++) {
		TP_REQUIRE(ctx, h_npix[i] >= 1 && h_npix[i] <= kMaxPitch, "tp_halo: npix must lie in [1, 4096]");
		TP_REQUIRE(ctx, h_ncad[i] >= 0, "tp_halo: negative ncad");
		TP_REQUIRE(ctx, h_p_offset[i] >= 0 && h_p_offset[i] % 4 == 0, "tp_halo: p_offset must be a non-negative multiple of 4");
	}
	return TP_OK;
}

} // namespace

extern "C" int tp_halo_tvmin(tp_ctx* ctx, int32_t n_problems, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad,
	const float* d_P, const uint8_t* d_fit, int32_t maxiter, int32_t history, double ftol, double gtol, double* d_w, double* d_l,
	double* d_f, int32_t* d_iters, int32_t* d_status)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	int rc = halo_check(ctx, n_problems, h_p_offset, h_npix, h_ncad, d_P, d_fit);
	if (rc != TP_OK || n_problems == 0) return rc;
	TP_REQUIRE(ctx, d_w && d_l && d_f && d_iters && d_status, "tp_halo_tvmin: null output pointer");
	TP_REQUIRE(ctx, maxiter >= 0 && history >= 1 && history <= kMaxHistory && ftol >= 0.0 && gtol >= 0.0, "tp_halo_tvmin: bad optimiser settings");
	return halo_run(ctx, n_problems, h_p_offset, h_npix, h_ncad, d_P, d_fit, nullptr, maxiter, history, ftol, gtol, 0, d_w, d_l, d_f, d_iters,
		d_status, nullptr);
	TP_API_END(ctx)
}

extern "C" int tp_halo_objective(tp_ctx* ctx, int32_t n_problems, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad,
	const float* d_P, const uint8_t* d_fit, const double* d_theta, double* d_f, double* d_grad)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	int rc = halo_check(ctx, n_problems, h_p_offset, h_npix, h_ncad, d_P, d_fit);
	if (rc != TP_OK || n_problems == 0) return rc;
	TP_REQUIRE(ctx, d_theta && d_f && d_grad, "tp_halo_objective: null pointer");
	return halo_run(ctx, n_problems, h_p_offset, h_npix, h_ncad, d_P, d_fit, d_theta, 0, 1, 0.0, 0.0, 1, nullptr, nullptr, d_f, nullptr, nullptr,
		d_grad);
	TP_API_END(ctx)
}

// ===============================================================================================================================
// The frames path: the problems of a batch of targets built on the device straight from a region's image stack
// (halo_photometry.py:118-123 the pixel mask handed in, :160-176 the segments, halophot's minflux cut and finite-cadence rule as
// restated in tests/halo_common.py::problems), and the outputs of :197-219 (normalised light curve, weight maps, flux error).
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
//   norm           (one block per problem): numpy's median of l over the fitted cadences (radix select over the 64-bit key, 256-bin
//                  integer histogram in LDS per pass) and the weight map w / median placed into the stamp;
//   lightcurve     (4 cadences per block, one wave each; target): corr_flux, flux, and flux_err as a fixed-order sum over the stamp.
// No float atomics anywhere: two runs give the same bits, and a target gives the same bits alone as inside a batch.
namespace {

constexpr int kSelTile = 64;          // cadences per select block
constexpr int kMaxStamp = 4096;       // pixels per stamp (a Halo stamp is 22 x 22)

struct StackGeom {
	int32_t n_frames, frame_rows, frame_cols, row0, col0, height, width, n_seg, n_targets;
};

__device__ inline uint32_t fkey(float v) {
	const uint32_t u = __float_as_uint(v);
	return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ inline float from_fkey(uint32_t k) {
	return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

// nanmedian(x.astype(float64)) < minflux from the counts: n non-NaN values, c of them < minflux, a the largest of those (key),
// b the smallest of the others (key).  Odd n: the middle value is below iff c >= (n + 1) / 2.  Even n: both middle values below
// (c >= n / 2 + 1), neither (c < n / 2), or a and b themselves: numpy's (a + b) / 2 in float64.  No value: NaN, not below.
__device__ inline bool drop_pixel(int32_t n, int32_t c, uint32_t akey, uint32_t bkey, double minflux) {
	if (n <= 0) return false;
	if (n & 1) return c >= (n + 1) / 2;
	if (c >= n / 2 + 1) return true;
	if (c < n / 2) return false;
	const double m = ((double)from_fkey(akey) + (double)from_fkey(bkey)) / 2.0;
	return m < minflux;
}

// image offset of stamp pixel p of a target inside one frame
__device__ inline int64_t stamp_offset(const StackGeom& g, const int32_t* st, int p) {
	return (int64_t)(st[0] - g.row0 + p / g.width) * g.frame_cols + (st[2] - g.col0 + p % g.width);
}

// tiles: int32 [n_tiles][3] = segment, first and one-past-last entry of cadlist; stats: int32 [4][n_prob * HW] = n, c, akey, bkey
__global__ __launch_bounds__(kThreads) void tp_halo_select_stat_kernel(StackGeom g, const float* __restrict__ images,
	const int32_t* __restrict__ stamps, const uint8_t* __restrict__ mask, const int32_t* __restrict__ tiles,
	const int32_t* __restrict__ cadlist, const uint8_t* __restrict__ fitlist, double minflux, int32_t* stats)
{
	const int i = blockIdx.y;
	const int k = tiles[3 * blockIdx.x], j0 = tiles[3 * blockIdx.x + 1], j1 = tiles[3 * blockIdx.x + 2];
	const int HW = g.height * g.width;
	const int64_t frame = (int64_t)g.frame_rows * g.frame_cols;
	const int64_t nstat = (int64_t)g.n_targets * g.n_seg * HW;
	const int64_t q = (int64_t)i * g.n_seg + k;
	const int32_t* st = stamps + 4 * i;
	for (int p = threadIdx.x; p < HW; p += kThreads) {
		if (!mask[(int64_t)i * HW + p]) continue;
		const int64_t off = stamp_offset(g, st, p);
		int32_t n = 0, c = 0;
		uint32_t ak = 0u, bk = 0xffffffffu;
		for (int j = j0; j < j1; j++) {
			if (!fitlist[j]) continue;
			const float x = images[(int64_t)cadlist[j] * frame + off];
			if (x != x) continue;
			n++;
			const uint32_t key = fkey(x);
			if ((double)x < minflux) { c++; ak = max(ak, key); }
			else bk = min(bk, key);
		}
		const int64_t s = q * HW + p;
		if (n) atomicAdd(&stats[s], n);
		if (c) atomicAdd(&stats[nstat + s], c);
		if (ak != 0u) atomicMax(reinterpret_cast<uint32_t*>(stats) + 2 * nstat + s, ak);
		if (bk != 0xffffffffu) atomicMin(reinterpret_cast<uint32_t*>(stats) + 3 * nstat + s, bk);
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
	const int i = blockIdx.y;
	const int k = tiles[3 * blockIdx.x], j0 = tiles[3 * blockIdx.x + 1], j1 = tiles[3 * blockIdx.x + 2];
	const int HW = g.height * g.width;
	const int64_t frame = (int64_t)g.frame_rows * g.frame_cols;
	const int64_t nstat = (int64_t)g.n_targets * g.n_seg * HW;
	const int64_t q = (int64_t)i * g.n_seg + k;
	const int32_t* st = stamps + 4 * i;
	const int first = seg_off[k];
	for (int p = threadIdx.x; p < HW; p += kThreads) {
		const int64_t s = q * HW + p;
		const bool kp = mask[(int64_t)i * HW + p] != 0 &&
			!drop_pixel(stats[s], stats[nstat + s], (uint32_t)stats[2 * nstat + s], (uint32_t)stats[3 * nstat + s], minflux);
		keep[p] = kp;
		if (j0 == first) pixkeep[s] = kp;
	}
	if (threadIdx.x < kSelTile) bad[threadIdx.x] = 0;
	__syncthreads();
	for (int p = threadIdx.x; p < HW; p += kThreads) {
		if (!keep[p]) continue;
		const int64_t off = stamp_offset(g, st, p);
		for (int j = j0; j < j1; j++) {
			const float x = images[(int64_t)cadlist[j] * frame + off];
			if (!(fabsf(x) <= 3.402823466e+38f)) bad[j - j0] = 1;   // NaN or infinite (every writer stores the same value)
		}
	}
	__syncthreads();
	for (int j = j0 + threadIdx.x; j < j1; j += kThreads) cadkeep[q * g.n_frames + (j - first)] = bad[j - j0] ? 0 : 1;
}

// ascending list of the set flags: out[rank] = value(index); returns the count (every thread)
template <class F> __device__ int compact_block(const uint8_t* flags, int n, int* wcount, F&& emit) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int base = 0;
	for (int c0 = 0; c0 < n; c0 += kThreads) {
		const int t = c0 + threadIdx.x;
		const bool flag = t < n && flags[t] != 0;
		const unsigned long long b = __ballot(flag);
		if (lane == 0) wcount[wave] = __popcll(b);
		__syncthreads();
		int before = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
		for (int k = 0; k < kThreads / 64; k++) {
			if (k < wave) before += wcount[k];
			total += wcount[k];
		}
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

struct GatherProb {
	int64_t p_off, c_off;
	int32_t q, npix, ncad, pitch;
};

constexpr int kGatherRows = 8;

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

struct NormProb {
	int64_t c_off, w_off;
	int32_t q, npix, ncad, pad;
};

// the key of rank `rank` (0-based, ascending) among the fitted l of one problem: eight passes of eight bits, most significant first
__device__ uint64_t select_rank(const double* l, const uint8_t* fit, int ncad, int rank, int* hist, uint64_t* found) {
	uint64_t prefix = 0;
	for (int shift = 56; shift >= 0; shift -= 8) {
		for (int b = threadIdx.x; b < 256; b += kThreads) hist[b] = 0;
		__syncthreads();
		for (int t = threadIdx.x; t < ncad; t += kThreads) {
			if (!fit[t]) continue;
			const uint64_t key = okey(l[t]);
			if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1);
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			int b = 0, r = rank;
			while (b < 255 && r >= hist[b]) { r -= hist[b]; b++; }
			found[0] = prefix | ((uint64_t)b << shift);
			found[1] = (uint64_t)r;
		}
		__syncthreads();
		prefix = found[0];
		rank = (int)found[1];
		__syncthreads();
	}
	return prefix;
}

// median double [n_prob] (NaN for a problem that was not run), weightmap double [n_prob][HW]; run: the run problem of q, or -1
__global__ __launch_bounds__(kThreads) void tp_halo_norm_kernel(StackGeom g, const int32_t* __restrict__ run, const NormProb* __restrict__ probs,
	const int32_t* __restrict__ pix, const uint8_t* __restrict__ fit, const double* __restrict__ w, const double* __restrict__ l,
	double* median, double* weightmap)
{
	__shared__ int hist[256];
	__shared__ uint64_t found[2];
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
	const double* myl = l + pr.c_off;
	const uint8_t* myfit = fit + pr.c_off;
	if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
	__syncthreads();
	int nf = 0, nn = 0;
	for (int t = threadIdx.x; t < pr.ncad; t += kThreads)
		if (myfit[t]) { nf++; nn += myl[t] != myl[t]; }
	if (nf) atomicAdd(&cnt[0], nf);
	if (nn) atomicAdd(&cnt[1], nn);
	__syncthreads();
	nf = cnt[0];
	nn = cnt[1];
	double med = NAN;   // numpy: the median of nothing, or of anything with a NaN, is NaN
	if (nf > 0 && nn == 0) {
		if (nf & 1) med = from_key(select_rank(myl, myfit, pr.ncad, nf / 2, hist, found));
		else {
			const double a = from_key(select_rank(myl, myfit, pr.ncad, nf / 2 - 1, hist, found));
			const double b = from_key(select_rank(myl, myfit, pr.ncad, nf / 2, hist, found));
			med = (a + b) / 2.0;
		}
	}
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
	double s = 0.0;
	for (int p = lane; p < HW; p += 64) {
		const double e = (double)err[stamp_offset(g, st, p)];
		const double term = (wm[p] * wm[p]) * (e * e);
		if (term == term) s += term;   // nansum
	}
	s = wave_sum(s);
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

int stack_check(tp_ctx* ctx, const StackGeom& g, const void* d_stack, const int32_t* h_stamps)
{
	TP_REQUIRE(ctx, d_stack && h_stamps, "tp_halo: null pointer");
	TP_REQUIRE(ctx, g.n_frames >= 1 && g.frame_rows >= 1 && g.frame_cols >= 1 && g.n_targets >= 1 && g.n_targets <= 65535, "tp_halo: bad stack or batch size");
	TP_REQUIRE(ctx, g.height >= 1 && g.width >= 1 && (int64_t)g.height * g.width <= kMaxStamp, "tp_halo: a stamp holds 1 .. 4096 pixels");
	TP_REQUIRE(ctx, g.n_seg >= 1 && g.n_seg <= 64, "tp_halo: 1 .. 64 segments");
	for (int i = 0; i < g.n_targets; i++) {
		const int32_t* s = h_stamps + 4 * i;
		TP_REQUIRE(ctx, s[1] - s[0] == g.height && s[3] - s[2] == g.width, "tp_halo: every stamp of a call has the call's height and width");
		TP_REQUIRE(ctx, s[0] >= g.row0 && s[1] <= g.row0 + g.frame_rows && s[2] >= g.col0 && s[3] <= g.col0 + g.frame_cols,
			"tp_halo: stamp outside the frame stack");
	}
	return TP_OK;
}

int seg_check(tp_ctx* ctx, const StackGeom& g, const int32_t* h_seg)
{
	TP_REQUIRE(ctx, h_seg, "tp_halo: null pointer");
	int32_t mx = -1;
	for (int t = 0; t < g.n_frames; t++) {
		TP_REQUIRE(ctx, h_seg[t] >= -1, "tp_halo: segment below -1");
		mx = std::max(mx, h_seg[t]);
	}
	TP_REQUIRE(ctx, mx + 1 == g.n_seg, "tp_halo: n_seg must be the largest segment plus one");
	return TP_OK;
}

struct DevBlocks {
	tp_ctx* ctx;
	std::vector<void*> ptrs;
	int rc = TP_OK;
	explicit DevBlocks(tp_ctx* c) : ctx(c) {}
	void* get(uint64_t bytes) {
		void* p = nullptr;
		if (rc == TP_OK) rc = tp_malloc(ctx, std::max<uint64_t>(bytes, 16), &p);
		if (p) ptrs.push_back(p);
		return p;
	}
	~DevBlocks() { for (void* p : ptrs) tp_free(ctx, p); }
};

} // namespace

extern "C" int tp_halo_select_stack(tp_ctx* ctx, const float* d_images, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int32_t row0,
	int32_t col0, int32_t n_targets, const int32_t* h_stamps, int32_t height, int32_t width, const uint8_t* d_mask, int32_t n_seg,
	const int32_t* h_seg, const int32_t* h_quality, int32_t bitmask, double minflux, int32_t* d_pix, int32_t* d_cad, uint8_t* d_fit,
	int32_t* d_cadpos, int32_t* d_npix, int32_t* d_ncad)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const StackGeom g{n_frames, frame_rows, frame_cols, row0, col0, height, width, n_seg, n_targets};
	int rc = stack_check(ctx, g, d_images, h_stamps);
	if (rc == TP_OK) rc = seg_check(ctx, g, h_seg);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, d_mask && h_quality && d_pix && d_cad && d_fit && d_cadpos && d_npix && d_ncad, "tp_halo_select_stack: null pointer");
	const int T = n_frames, HW = height * width;
	const int64_t n_prob = (int64_t)n_targets * n_seg;
	// the cadences of every segment in ascending order, their fit flags, and the tiles of kSelTile of them
	std::vector<int32_t> cadlist, seg_off(n_seg + 1, 0), tiles;
	std::vector<uint8_t> fitlist;
	for (int k = 0; k < n_seg; k++) {
		for (int t = 0; t < T; t++)
			if (h_seg[t] == k) {
				cadlist.push_back(t);
				fitlist.push_back((h_quality[t] & bitmask) == 0);
			}
		seg_off[k + 1] = (int32_t)cadlist.size();
		for (int j = seg_off[k]; j < seg_off[k + 1]; j += kSelTile) {
			tiles.push_back(k);
			tiles.push_back(j);
			tiles.push_back(std::min(j + kSelTile, seg_off[k + 1]));
		}
	}
	const unsigned n_tiles = (unsigned)(tiles.size() / 3);
	DevBlocks dev(ctx);
	int32_t* dstamps = (int32_t*)dev.get((uint64_t)n_targets * 4 * sizeof(int32_t));
	int32_t* dcadlist = (int32_t*)dev.get(cadlist.size() * sizeof(int32_t));
	uint8_t* dfitlist = (uint8_t*)dev.get(fitlist.size());
	int32_t* dsegoff = (int32_t*)dev.get(seg_off.size() * sizeof(int32_t));
	int32_t* dtiles = (int32_t*)dev.get(tiles.size() * sizeof(int32_t));
	int32_t* dstats = (int32_t*)dev.get((uint64_t)n_prob * HW * 4 * sizeof(int32_t));
	uint8_t* dpixkeep = (uint8_t*)dev.get((uint64_t)n_prob * HW);
	uint8_t* dcadkeep = (uint8_t*)dev.get((uint64_t)n_prob * T);
	if (dev.rc != TP_OK) return dev.rc;
	hipStream_t s = ctx->stream;
	TP_HIP(ctx, hipMemcpyAsync(dstamps, h_stamps, (size_t)n_targets * 4 * sizeof(int32_t), hipMemcpyHostToDevice, s));
	if (!cadlist.empty()) {
		TP_HIP(ctx, hipMemcpyAsync(dcadlist, cadlist.data(), cadlist.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
		TP_HIP(ctx, hipMemcpyAsync(dfitlist, fitlist.data(), fitlist.size(), hipMemcpyHostToDevice, s));
		TP_HIP(ctx, hipMemcpyAsync(dtiles, tiles.data(), tiles.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
	}
	TP_HIP(ctx, hipMemcpyAsync(dsegoff, seg_off.data(), seg_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
	const size_t stat_bytes = (size_t)n_prob * HW * sizeof(int32_t);
	TP_HIP(ctx, hipMemsetAsync(dstats, 0, 3 * stat_bytes, s));
	TP_HIP(ctx, hipMemsetAsync(reinterpret_cast<char*>(dstats) + 3 * stat_bytes, 0xff, stat_bytes, s));
	TP_HIP(ctx, hipMemsetAsync(dpixkeep, 0, (size_t)n_prob * HW, s));
	TP_HIP(ctx, hipMemsetAsync(d_cadpos, 0xff, (size_t)n_targets * T * sizeof(int32_t), s));
	if (n_tiles) {
		TP_LAUNCH(ctx, TPK_HALO_SELECT_STAT, tp_halo_select_stat_kernel, dim3(n_tiles, (unsigned)n_targets), dim3(kThreads), 0, g, d_images,
			(const int32_t*)dstamps, d_mask, (const int32_t*)dtiles, (const int32_t*)dcadlist, (const uint8_t*)dfitlist, minflux, dstats);
		TP_LAUNCH_CHECK(ctx, "tp_halo_select_stat_kernel");
		TP_LAUNCH(ctx, TPK_HALO_SELECT_CAD, tp_halo_select_cad_kernel, dim3(n_tiles, (unsigned)n_targets), dim3(kThreads), 0, g, d_images,
			(const int32_t*)dstamps, d_mask, (const int32_t*)dtiles, (const int32_t*)dcadlist, (const int32_t*)dsegoff, minflux,
			(const int32_t*)dstats, dpixkeep, dcadkeep);
		TP_LAUNCH_CHECK(ctx, "tp_halo_select_cad_kernel");
	}
	TP_LAUNCH(ctx, TPK_HALO_SELECT_COMPACT, tp_halo_select_compact_kernel, dim3((unsigned)n_prob), dim3(kThreads), 0, g, (const int32_t*)dcadlist,
		(const uint8_t*)dfitlist, (const int32_t*)dsegoff, d_mask, (const uint8_t*)dpixkeep, (const uint8_t*)dcadkeep, d_pix, d_cad, d_fit,
		d_cadpos, d_npix, d_ncad);
	TP_LAUNCH_CHECK(ctx, "tp_halo_select_compact_kernel");
	TP_HIP(ctx, hipStreamSynchronize(s));   // the host vectors the asynchronous copies read must outlive them
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
	int rc = stack_check(ctx, g, d_images, h_stamps);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, n_run >= 0 && n_run <= 65535, "tp_halo_gather_stack: 0 .. 65535 problems per call");
	if (n_run == 0) return TP_OK;
	TP_REQUIRE(ctx, d_pix && d_cad && d_fit && h_index && h_p_offset && h_npix && h_ncad && d_P && d_fit_out, "tp_halo_gather_stack: null pointer");
	const int HW = height * width;
	std::vector<GatherProb> probs(n_run);
	int64_t c_tot = 0;
	int32_t max_ncad = 0;
	for (int r = 0; r < n_run; r++) {
		TP_REQUIRE(ctx, h_index[r] >= 0 && h_index[r] < (int64_t)n_targets * n_seg, "tp_halo_gather_stack: problem index out of range");
		TP_REQUIRE(ctx, h_npix[r] >= 1 && h_npix[r] <= HW && h_ncad[r] >= 0 && h_ncad[r] <= n_frames, "tp_halo_gather_stack: npix or ncad out of range");
		TP_REQUIRE(ctx, h_p_offset[r] >= 0 && h_p_offset[r] % 4 == 0, "tp_halo_gather_stack: p_offset must be a non-negative multiple of 4");
		probs[r] = GatherProb{h_p_offset[r], c_tot, h_index[r], h_npix[r], h_ncad[r], (h_npix[r] + 3) & ~3};
		c_tot += h_ncad[r];
		max_ncad = std::max(max_ncad, h_ncad[r]);
	}
	if (max_ncad == 0) return TP_OK;
	DevBlocks dev(ctx);
	int32_t* dstamps = (int32_t*)dev.get((uint64_t)n_targets * 4 * sizeof(int32_t));
	GatherProb* dprobs = (GatherProb*)dev.get((uint64_t)n_run * sizeof(GatherProb));
	if (dev.rc != TP_OK) return dev.rc;
	hipStream_t s = ctx->stream;
	TP_HIP(ctx, hipMemcpyAsync(dstamps, h_stamps, (size_t)n_targets * 4 * sizeof(int32_t), hipMemcpyHostToDevice, s));
	TP_HIP(ctx, hipMemcpyAsync(dprobs, probs.data(), (size_t)n_run * sizeof(GatherProb), hipMemcpyHostToDevice, s));
	TP_LAUNCH(ctx, TPK_HALO_GATHER, tp_halo_gather_kernel, dim3((unsigned)((max_ncad + kGatherRows - 1) / kGatherRows), (unsigned)n_run), dim3(kThreads), 0,
		g, d_images, (const int32_t*)dstamps, (const GatherProb*)dprobs, d_pix, d_cad, d_fit, d_P, d_fit_out);
	TP_LAUNCH_CHECK(ctx, "tp_halo_gather_kernel");
	TP_HIP(ctx, hipStreamSynchronize(s));
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
	int rc = stack_check(ctx, g, d_images_err, h_stamps);
	if (rc == TP_OK) rc = seg_check(ctx, g, h_seg);
	if (rc != TP_OK) return rc;
	TP_REQUIRE(ctx, n_run >= 0 && n_run <= 65535, "tp_halo_outputs_stack: 0 .. 65535 problems per call");
	TP_REQUIRE(ctx, d_pix && d_cadpos && h_normfactor && d_median && d_corr && d_flux && d_flux_err && d_weightmap, "tp_halo_outputs_stack: null pointer");
	TP_REQUIRE(ctx, n_run == 0 || (h_index && h_npix && h_ncad && d_fit && d_w && d_l && d_status), "tp_halo_outputs_stack: null pointer");
	const int HW = height * width;
	const int64_t n_prob = (int64_t)n_targets * n_seg;
	std::vector<NormProb> probs(std::max(n_run, 1));
	std::vector<int32_t> run(n_prob, -1);
	int64_t c_tot = 0, w_tot = 0;
	for (int r = 0; r < n_run; r++) {
		TP_REQUIRE(ctx, h_index[r] >= 0 && h_index[r] < n_prob && run[h_index[r]] < 0, "tp_halo_outputs_stack: bad problem index");
		TP_REQUIRE(ctx, h_npix[r] >= 1 && h_npix[r] <= HW && h_ncad[r] >= 0 && h_ncad[r] <= n_frames, "tp_halo_outputs_stack: npix or ncad out of range");
		probs[r] = NormProb{c_tot, w_tot, h_index[r], h_npix[r], h_ncad[r], 0};
		run[h_index[r]] = r;
		c_tot += h_ncad[r];
		w_tot += h_npix[r];
	}
	DevBlocks dev(ctx);
	int32_t* dstamps = (int32_t*)dev.get((uint64_t)n_targets * 4 * sizeof(int32_t));
	NormProb* dprobs = (NormProb*)dev.get(probs.size() * sizeof(NormProb));
	int32_t* drun = (int32_t*)dev.get((uint64_t)n_prob * sizeof(int32_t));
	int32_t* dseg = (int32_t*)dev.get((uint64_t)n_frames * sizeof(int32_t));
	double* dnorm = (double*)dev.get((uint64_t)n_targets * sizeof(double));
	if (dev.rc != TP_OK) return dev.rc;
	hipStream_t s = ctx->stream;
	TP_HIP(ctx, hipMemcpyAsync(dstamps, h_stamps, (size_t)n_targets * 4 * sizeof(int32_t), hipMemcpyHostToDevice, s));
	TP_HIP(ctx, hipMemcpyAsync(dprobs, probs.data(), probs.size() * sizeof(NormProb), hipMemcpyHostToDevice, s));
	TP_HIP(ctx, hipMemcpyAsync(drun, run.data(), (size_t)n_prob * sizeof(int32_t), hipMemcpyHostToDevice, s));
	TP_HIP(ctx, hipMemcpyAsync(dseg, h_seg, (size_t)n_frames * sizeof(int32_t), hipMemcpyHostToDevice, s));
	TP_HIP(ctx, hipMemcpyAsync(dnorm, h_normfactor, (size_t)n_targets * sizeof(double), hipMemcpyHostToDevice, s));
	TP_LAUNCH(ctx, TPK_HALO_NORM, tp_halo_norm_kernel, dim3((unsigned)n_prob), dim3(kThreads), 0, g, (const int32_t*)drun, (const NormProb*)dprobs,
		d_pix, d_fit, d_w, d_l, d_median, d_weightmap);
	TP_LAUNCH_CHECK(ctx, "tp_halo_norm_kernel");
	TP_LAUNCH(ctx, TPK_HALO_LIGHTCURVE, tp_halo_lightcurve_kernel, dim3((unsigned)((n_frames + kThreads / 64 - 1) / (kThreads / 64)), (unsigned)n_targets),
		dim3(kThreads), 0, g, d_images_err, (const int32_t*)dstamps, (const int32_t*)dseg, (const int32_t*)drun, (const NormProb*)dprobs, d_cadpos,
		d_l, d_status, (const double*)d_median, (const double*)d_weightmap, (const double*)dnorm, d_corr, d_flux, d_flux_err);
	TP_LAUNCH_CHECK(ctx, "tp_halo_lightcurve_kernel");
	TP_HIP(ctx, hipStreamSynchronize(s));
	return TP_OK;
	TP_API_END(ctx)
}
