// halo.hip -- Halo photometry (photometry/halo/halo_photometry.py:86-265) on the device: the TV-min pixel weights of Pope et al.
// (2016, 2019) for a batch of problems (one problem = one light-curve segment of one target).  The frames path that builds the
// problems from a region's image stack is halo_stack.hip.
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
// What a step decides -- every transition of the state, every rule with a constant -- is halo_rules.h; the reductions and the
// selection are halo_dev.h; the kernels here are the parallel plumbing around them.
// The host loop polls the problem states and relaunches over the problems still active (as csrc/motion.hip).  No float atomics:
// every reduction has a fixed order, so a problem gives the same bits alone as inside a batch.
#include "halo_dev.h"

namespace {

using namespace tp_halo;

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

// ---- init: fitted-cadence list, sign terms zeroed, theta, w, state ---------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tp_halo_init_kernel(HaloArgs a, const double* theta_in)
{
	const int pi = blockIdx.x;
	const HaloProb pr = a.prob[pi];
	__shared__ double red[kThreads / 64];
	__shared__ int wcount[kThreads / 64];
	int base = 0;
	for (int c0 = 0; c0 < pr.ncad; c0 += kThreads) {
		const int t = c0 + threadIdx.x;
		const bool flag = t < pr.ncad && a.fit[pr.c_off + t] != 0;
		if (t < pr.ncad) a.sgn[pr.c_off + t] = 0.0f;
		int total;
		const int before = block_rank<kThreads>(flag, wcount, total);
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
	if (threadIdx.x == 0) state_init(a.state[pi], base);
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
// the fitted light curve of a problem: l_F[j] = l[fidx[j]], j < nf
struct Fitted {
	const double* l;
	const int32_t* fidx;
	int nf;
	__device__ double at(int j) const { return l[fidx[j]]; }
};

struct StatShared {
	int hist[256];
	int sh[4];
	int wcount[kStatThreads / 64];
	double red[kStatThreads / 64];
};

// TV and the sign terms s_t (the ends have one neighbour)
__device__ double stat_tv_and_signs(const Fitted& F, float* sgn, double* red) {
	double tv = 0.0;
	for (int j = threadIdx.x; j < F.nf; j += kStatThreads) {
		const double v = F.at(j);
		const double dp = j > 0 ? v - F.at(j - 1) : 0.0;
		const double dn = j + 1 < F.nf ? F.at(j + 1) - v : 0.0;
		sgn[F.fidx[j]] = sign_term(dp, dn);
		tv += fabs(dn);
	}
	return block_sum<kStatThreads>(tv, red);
}

// the key of rank k of l_F: the thread's keys are the cached ones and, beyond kKR * kStatThreads fitted cadences, re-read ones
__device__ __forceinline__ Select stat_select(const uint64_t (&kc)[kKR], const Fitted& F, int k, StatShared& s) {
	return block_radix_select<kStatThreads>([&](auto&& visit) {
#pragma unroll
		for (int r = 0; r < kKR; r++)
			if (r * kStatThreads + (int)threadIdx.x < F.nf) visit(kc[r]);
		for (int j = kKR * kStatThreads + (int)threadIdx.x; j < F.nf; j += kStatThreads) visit(okey(F.at(j)));
	}, k, s.hist, s.sh);
}

// the cadence (problem-local index) of the rank-th occurrence, in time order, of the key among the fitted l
__device__ int find_occurrence(const Fitted& F, Select sel, StatShared& s) {
	int rank = sel.rank;
	if (threadIdx.x == 0) s.sh[2] = -1;
	__syncthreads();
	for (int base = 0; base < F.nf; base += kStatThreads) {
		const int j = base + (int)threadIdx.x;
		const bool match = j < F.nf && okey(F.at(j)) == sel.key;
		int total;
		const int before = block_rank<kStatThreads>(match, s.wcount, total);
		if (match && before == rank) s.sh[2] = F.fidx[j];
		__syncthreads();
		if (s.sh[2] >= 0) break;
		rank -= total;
	}
	const int r = s.sh[2];
	__syncthreads();
	return r;
}

__global__ __launch_bounds__(kStatThreads) void tp_halo_stat_kernel(HaloArgs a, const int32_t* __restrict__ plist)
{
	const int pi = plist[blockIdx.x];
	const HaloState st = a.state[pi];
	if (st.status != ST_ACTIVE) return;
	const HaloProb pr = a.prob[pi];
	__shared__ StatShared s;
	const Fitted F{a.l + pr.c_off, a.fidx + pr.c_off, st.nf};
	uint64_t kc[kKR];
#pragma unroll
	for (int r = 0; r < kKR; r++) {
		const int j = r * kStatThreads + (int)threadIdx.x;
		kc[r] = j < F.nf ? okey(F.at(j)) : 0;
	}
	const double tv = stat_tv_and_signs(F, a.sgn + pr.c_off, s.red);
	// the median
	const int k1 = mid_lo(F.nf), k2 = mid_hi(F.nf);
	const Select s1 = stat_select(kc, F, k1, s);
	Select s2 = s1;
	if (k2 != k1) s2 = stat_select(kc, F, k2, s);
	const double m = median_of_keys(s1.key, s2.key, k2 != k1);
	const bool valid = median_valid(m);
	const double ft = objective_value(tv, m, valid);
	// the decision (uniform over the block), then publish or the next trial
	HaloState& so = a.state[pi];
	switch (stat_decide(st, ft, valid)) {
	case kStatAccept: {
		const int t0 = find_occurrence(F, s1, s);
		const int t1 = k2 != k1 ? find_occurrence(F, s2, s) : t0;
		if (threadIdx.x == 0) stat_accept(so, st, ft, m, t0, t1);
		break;
	}
	case kStatDegenerate:
		if (threadIdx.x == 0) stat_degenerate(so);
		break;
	case kStatLineSearchFailed:
		if (threadIdx.x == 0) stat_line_search_failed(so, st);
		break;
	default: {
		const double alpha = next_alpha(st);
		softmax_into<kStatThreads>(a.theta + pr.w_off, a.d + pr.w_off, alpha, pr.npix, pr.pitch, a.w + pr.w_off, s.red);
		if (threadIdx.x == 0) stat_next_trial(so, st, alpha);
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
struct FinishShared {
	double red[kThreads / 64];
	double sa[kMaxHistory], ssy[kMaxHistory], syy[kMaxHistory];   // alpha_i of the two-loop recursion; s.y and y.y per slot
};

// the arrays of one problem
struct FinishView {
	int npix, pitch, ntiles, H;
	const float* P;
	const double* part;
	double *th, *g, *d, *w, *q, *S, *Y, *pairs;
};

__device__ FinishView finish_view(const HaloArgs& a, const HaloProb& pr, int pi) {
	return FinishView{pr.npix, pr.pitch, pr.ntiles, a.history, a.P + pr.p_off, a.partial + pr.part_off, a.theta + pr.w_off, a.g + pr.w_off,
		a.d + pr.w_off, a.w + pr.w_off, a.q + pr.w_off, a.S ? a.S + pr.h_off : nullptr, a.Y ? a.Y + pr.h_off : nullptr, a.pairs ? a.pairs + (int64_t)pi * kMaxHistory * 2 : nullptr};
}

// q = gradient with respect to w, from the tile partials and the median row; returns w.q
__device__ double finish_gradient(const FinishView& v, const HaloState& st, double* red) {
	const double m = st.m, fm = st.f / m;
	const float* r0 = v.P + (int64_t)st.tmed0 * v.pitch;
	const float* r1 = v.P + (int64_t)st.tmed1 * v.pitch;
	double acc = 0.0;
	for (int p = threadIdx.x; p < v.npix; p += kThreads) {
		const double G = sum_tiles(v.ntiles, [&](int t) { return v.part[(int64_t)t * v.pitch + p]; });
		const double gw = grad_w(G, m, fm, median_row(r0, r1, st.tmed0 == st.tmed1, p));
		v.q[p] = gw;
		acc += v.w[p] * gw;
	}
	return block_sum<kThreads>(acc, red);
}

// through the softmax: q = w (q - w.q); returns |q|_inf
__device__ double finish_softmax_chain(const FinishView& v, double wg, double* red) {
	double gmax = 0.0;
	for (int p = threadIdx.x; p < v.npix; p += kThreads) {
		const double gt = v.w[p] * (v.q[p] - wg);
		v.q[p] = gt;
		gmax = fmax(gmax, fabs(gt));
	}
	return block_max<kThreads>(gmax, red);
}

// s = theta_new - theta, y = grad_new - grad: the pair stored if the rule keeps it, then theta and g moved on to the new point
__device__ void finish_pair_update(const FinishView& v, double alpha, FinishShared& s, int& n_pairs, int& newest) {
	double sy = 0.0, yy = 0.0;
	for (int p = threadIdx.x; p < v.npix; p += kThreads) {
		const double tn = v.th[p] + alpha * v.d[p];
		const double sp = tn - v.th[p], y = v.q[p] - v.g[p];
		sy += sp * y;
		yy += y * y;
	}
	sy = block_sum<kThreads>(sy, s.red);
	yy = block_sum<kThreads>(yy, s.red);
	const bool keep = pair_kept(sy, yy);
	const int slot = next_slot(newest, v.H);
	double* Sk = v.S + (int64_t)slot * v.pitch;
	double* Yk = v.Y + (int64_t)slot * v.pitch;
	for (int p = threadIdx.x; p < v.npix; p += kThreads) {
		const double tn = v.th[p] + alpha * v.d[p];
		if (keep) {
			Sk[p] = tn - v.th[p];
			Yk[p] = v.q[p] - v.g[p];
		}
		v.th[p] = tn;
		v.g[p] = v.q[p];
	}
	if (keep) {
		pair_stored(slot, v.H, n_pairs, newest);
		if (threadIdx.x == 0) {
			s.ssy[slot] = sy;
			s.syy[slot] = yy;
			v.pairs[2 * slot] = sy;
			v.pairs[2 * slot + 1] = yy;
		}
	}
}

// d = -H g by the two-loop recursion over the pairs (oldest .. newest); returns g.d
__device__ double finish_two_loop(const FinishView& v, FinishShared& s, int n_pairs, int newest) {
	for (int p = threadIdx.x; p < v.npix; p += kThreads) v.d[p] = v.g[p];
	for (int i = n_pairs - 1; i >= 0; i--) {
		const int k = pair_slot(newest, n_pairs, i, v.H);
		const double* Sk = v.S + (int64_t)k * v.pitch;
		const double* Yk = v.Y + (int64_t)k * v.pitch;
		double x = 0.0;
		for (int p = threadIdx.x; p < v.npix; p += kThreads) x += Sk[p] * v.d[p];
		const double ai = (1.0 / s.ssy[k]) * block_sum<kThreads>(x, s.red);
		if (threadIdx.x == 0) s.sa[i] = ai;
		for (int p = threadIdx.x; p < v.npix; p += kThreads) v.d[p] -= ai * Yk[p];
	}
	const double gamma = gamma_of(s.ssy[newest], s.syy[newest]);
	for (int p = threadIdx.x; p < v.npix; p += kThreads) v.d[p] = gamma * v.d[p];
	__syncthreads();
	for (int i = 0; i < n_pairs; i++) {
		const int k = pair_slot(newest, n_pairs, i, v.H);
		const double* Sk = v.S + (int64_t)k * v.pitch;
		const double* Yk = v.Y + (int64_t)k * v.pitch;
		double x = 0.0;
		for (int p = threadIdx.x; p < v.npix; p += kThreads) x += Yk[p] * v.d[p];
		const double b = (1.0 / s.ssy[k]) * block_sum<kThreads>(x, s.red);
		const double ai = s.sa[i];
		for (int p = threadIdx.x; p < v.npix; p += kThreads) v.d[p] += Sk[p] * (ai - b);
	}
	double x = 0.0;
	for (int p = threadIdx.x; p < v.npix; p += kThreads) {
		v.d[p] = -v.d[p];
		x += v.g[p] * v.d[p];
	}
	return block_sum<kThreads>(x, s.red);
}

// d = -g / |g|_2; returns g.d
__device__ double finish_steepest_descent(const FinishView& v, double* red) {
	double x = 0.0;
	for (int p = threadIdx.x; p < v.npix; p += kThreads) x += v.g[p] * v.g[p];
	const double nrm = sqrt(block_sum<kThreads>(x, red));
	x = 0.0;
	for (int p = threadIdx.x; p < v.npix; p += kThreads) {
		v.d[p] = -v.g[p] / nrm;
		x += v.g[p] * v.d[p];
	}
	return block_sum<kThreads>(x, red);
}

__global__ __launch_bounds__(kThreads) void tp_halo_finish_kernel(HaloArgs a, const int32_t* __restrict__ plist)
{
	const int pi = plist[blockIdx.x];
	const HaloState st = a.state[pi];
	if (st.status != ST_ACTIVE || !st.need_grad) return;
	const HaloProb pr = a.prob[pi];
	__shared__ FinishShared s;
	const FinishView v = finish_view(a, pr, pi);
	if (v.pairs && threadIdx.x < v.H) {
		s.ssy[threadIdx.x] = v.pairs[2 * threadIdx.x];
		s.syy[threadIdx.x] = v.pairs[2 * threadIdx.x + 1];
	}
	const double wg = finish_gradient(v, st, s.red);
	const double gmax = finish_softmax_chain(v, wg, s.red);
	HaloState& so = a.state[pi];
	int status, n_pairs = st.n_pairs, newest = st.newest;
	if (st.initial) {
		if (a.objective) {   // the objective-only exit: the gradient is the answer
			for (int p = threadIdx.x; p < v.npix; p += kThreads) a.grad_out[pr.o_off + p] = v.q[p];
			if (threadIdx.x == 0) finish_objective(so);
			return;
		}
		for (int p = threadIdx.x; p < v.npix; p += kThreads) v.g[p] = v.q[p];
		status = stop_initial(gmax, a.gtol, a.maxiter);
	} else {
		finish_pair_update(v, st.alpha, s, n_pairs, newest);
		status = stop_step(st.f_prev, st.f, gmax, st.iters, a.ftol, a.gtol, a.maxiter);
	}
	__syncthreads();   // the scalars of the new pair visible to every thread
	if (status != ST_ACTIVE) {
		if (threadIdx.x == 0) finish_stopped(so, status, n_pairs, newest);
		return;
	}
	double gtd = 0.0;
	if (n_pairs > 0) {
		gtd = finish_two_loop(v, s, n_pairs, newest);
		if (!is_descent(gtd)) n_pairs = 0;
	}
	if (n_pairs == 0) gtd = finish_steepest_descent(v, s.red);
	softmax_into<kThreads>(v.th, v.d, 1.0, v.npix, v.pitch, v.w, s.red);
	if (threadIdx.x == 0) finish_next_search(so, gtd, n_pairs, newest);
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

// ---- the host loop ---------------------------------------------------------------------------------------------------------
struct SolverSettings {
	int32_t maxiter, history;
	double ftol, gtol;
	int32_t objective;
};

// one call's device workspace and what the loop keeps on the host
struct SolverRun {
	tp_ctx* ctx;
	const SolverLayout& L;
	HaloArgs a{};
	HaloProb* dprob = nullptr;
	int32_t *dlist2 = nullptr, *dplist = nullptr;
	std::vector<HaloState> states;        // as last read back
	std::vector<int32_t> list2, plist;    // the launch lists (the asynchronous copies read them: they live as long as the run)
	size_t lds() const { return (size_t)L.max_pitch * sizeof(double); }
};

int solver_workspace(SolverRun& r, DevBlocks& dev, const SolverSettings& s, const float* d_P, const uint8_t* d_fit, double* d_l, double* d_grad)
{
	const SolverLayout& L = r.L;
	const uint64_t n = L.prob.size();
	HaloArgs& a = r.a;
	r.dprob = dev.get<HaloProb>(n);
	a.prob = r.dprob;
	a.state = dev.get<HaloState>(n);
	a.P = d_P;
	a.fit = d_fit;
	a.l = d_l ? d_l : dev.get<double>(L.c_tot);
	a.fidx = dev.get<int32_t>(L.c_tot);
	a.sgn = dev.get<float>(L.c_tot);
	double* pix = dev.get<double>((uint64_t)L.w_tot * 5);
	a.theta = pix; a.g = pix + L.w_tot; a.d = pix + 2 * L.w_tot; a.w = pix + 3 * L.w_tot; a.q = pix + 4 * L.w_tot;
	a.S = s.objective ? nullptr : dev.get<double>((uint64_t)L.w_tot * s.history * 2);
	a.Y = a.S ? a.S + L.w_tot * s.history : nullptr;
	a.pairs = s.objective ? nullptr : dev.get<double>(n * kMaxHistory * 2);
	a.partial = dev.get<double>(L.part_tot);
	r.dlist2 = dev.get<int32_t>((uint64_t)L.tiles_tot * 2);
	r.dplist = dev.get<int32_t>(n);
	a.maxiter = s.maxiter;
	a.history = s.history;
	a.ftol = s.ftol;
	a.gtol = s.gtol;
	a.objective = s.objective;
	a.grad_out = d_grad;
	return dev.rc;
}

// the states from the device, and the launch lists over the problems still active
int solver_poll(SolverRun& r)
{
	tp_ctx* ctx = r.ctx;
	r.states.resize(r.L.prob.size());
	TP_HIP(ctx, hipMemcpyAsync(r.states.data(), r.a.state, r.states.size() * sizeof(HaloState), hipMemcpyDeviceToHost, ctx->stream));
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	launch_lists(r.L.prob, r.states.data(), r.list2, r.plist);
	return TP_OK;
}

// the problem table and the initial states (degenerate problems never start)
int solver_start(SolverRun& r, const double* d_theta)
{
	tp_ctx* ctx = r.ctx;
	const size_t n = r.L.prob.size();
	TP_HIP(ctx, hipMemcpyAsync(r.dprob, r.L.prob.data(), n * sizeof(HaloProb), hipMemcpyHostToDevice, ctx->stream));
	TP_LAUNCH(ctx, TPK_HALO_INIT, tp_halo_init_kernel, dim3((unsigned)n), dim3(kThreads), 0, r.a, d_theta);
	TP_LAUNCH_CHECK(ctx, "tp_halo_init_kernel");
	return solver_poll(r);
}

// the step loop: `poll` steps over the active problems, then a look at the states
int solver_steps(SolverRun& r)
{
	tp_ctx* ctx = r.ctx;
	const int64_t limit = max_steps(r.a.objective, r.a.maxiter);
	int64_t done = 0;
	int32_t poll = first_poll(r.a.objective);
	while (!r.plist.empty() && done < limit) {
		TP_HIP(ctx, hipMemcpyAsync(r.dlist2, r.list2.data(), r.list2.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
		TP_HIP(ctx, hipMemcpyAsync(r.dplist, r.plist.data(), r.plist.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
		const unsigned nt = (unsigned)(r.list2.size() / 2), np = (unsigned)r.plist.size();
		const int64_t steps = std::min<int64_t>(poll, limit - done);
		for (int64_t s = 0; s < steps; s++) {
			TP_LAUNCH(ctx, TPK_HALO_FORWARD, tp_halo_forward_kernel, dim3(nt), dim3(kThreads), r.lds(), r.a, (const int32_t*)r.dlist2, 0);
			TP_LAUNCH(ctx, TPK_HALO_STAT, tp_halo_stat_kernel, dim3(np), dim3(kStatThreads), 0, r.a, (const int32_t*)r.dplist);
			TP_LAUNCH(ctx, TPK_HALO_BACKWARD, tp_halo_backward_kernel, dim3(nt), dim3(kThreads), 0, r.a, (const int32_t*)r.dlist2);
			TP_LAUNCH(ctx, TPK_HALO_FINISH, tp_halo_finish_kernel, dim3(np), dim3(kThreads), 0, r.a, (const int32_t*)r.dplist);
		}
		TP_LAUNCH_CHECK(ctx, "tp_halo_forward_kernel");
		done += steps;
		const int rc = solver_poll(r);
		if (rc != TP_OK) return rc;
		poll = next_poll(poll);
	}
	return TP_OK;
}

// w, f, iterations and status; l at every cadence of every problem where the caller asks for it
int solver_outputs(SolverRun& r, double* d_w, double* d_l, double* d_f, int32_t* d_iters, int32_t* d_status)
{
	tp_ctx* ctx = r.ctx;
	TP_LAUNCH(ctx, TPK_HALO_OUTPUT, tp_halo_output_kernel, dim3((unsigned)r.L.prob.size()), dim3(kThreads), 0, r.a, d_w, d_f, d_iters, d_status);
	if (d_l) {
		launch_lists(r.L.prob, nullptr, r.list2, r.plist);
		if (!r.list2.empty()) {
			TP_HIP(ctx, hipMemcpyAsync(r.dlist2, r.list2.data(), r.list2.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
			TP_LAUNCH(ctx, TPK_HALO_FORWARD, tp_halo_forward_kernel, dim3((unsigned)(r.list2.size() / 2)), dim3(kThreads), r.lds(), r.a,
				(const int32_t*)r.dlist2, 1);
		}
	}
	TP_LAUNCH_CHECK(ctx, "tp_halo_output_kernel");
	// the host vectors the asynchronous copies read must outlive them
	TP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return TP_OK;
}

// layout, workspace, initial states, the step loop, outputs
int halo_run(tp_ctx* ctx, int32_t n, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad, const float* d_P,
	const uint8_t* d_fit, const double* d_theta, const SolverSettings& s, double* d_w, double* d_l, double* d_f, int32_t* d_iters,
	int32_t* d_status, double* d_grad)
{
	const SolverLayout L = solver_layout(n, h_p_offset, h_npix, h_ncad, s.history);
	const char* bad = solver_layout_check(L);
	TP_REQUIRE(ctx, !bad, bad);
	DevBlocks dev(ctx);
	SolverRun r{ctx, L};
	int rc = solver_workspace(r, dev, s, d_P, d_fit, d_l, d_grad);
	if (rc == TP_OK) rc = solver_start(r, d_theta);
	if (rc == TP_OK) rc = solver_steps(r);
	if (rc == TP_OK) rc = solver_outputs(r, d_w, d_l, d_f, d_iters, d_status);
	return rc;
}

int halo_check(tp_ctx* ctx, int32_t n, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad, const float* d_P, const uint8_t* d_fit)
{
	const char* bad = solver_check(n, h_p_offset, h_npix, h_ncad, d_P, d_fit);
	TP_REQUIRE(ctx, !bad, bad);
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
	TP_REQUIRE(ctx, settings_ok(maxiter, history, ftol, gtol), "tp_halo_tvmin: bad optimiser settings");
	return halo_run(ctx, n_problems, h_p_offset, h_npix, h_ncad, d_P, d_fit, nullptr, SolverSettings{maxiter, history, ftol, gtol, 0}, d_w, d_l, d_f,
		d_iters, d_status, nullptr);
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
	return halo_run(ctx, n_problems, h_p_offset, h_npix, h_ncad, d_P, d_fit, d_theta, SolverSettings{0, 1, 0.0, 0.0, 1}, nullptr, nullptr, d_f, nullptr,
		nullptr, d_grad);
	TP_API_END(ctx)
}
