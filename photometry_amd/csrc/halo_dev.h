// halo_dev.h -- the parallel plumbing of Halo photometry's kernels (halo.hip, halo_stack.hip, halo_cubes.hip), once each: fixed-order reductions,
// the softmax, the ballot-ordered rank of a flag inside a block and the radix selection of a rank.  What they compute is decided in
// halo_rules.h.  No float atomics: every reduction has a fixed order.  Also DevBlocks, the device blocks of one host entry.
#pragma once
#include "common.h"
#include "halo_rules.h"

namespace tp_halo {

__device__ inline double wave_sum(double v) {
	for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}
__device__ inline double wave_max(double v) {
	for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
	return v;
}

// numpy's pairwise add.reduce over term(0) .. term(n - 1) -- what np.nansum does once the NaNs are replaced (loops_utils.h.src) --
// by a whole wavefront, bit for bit: a leaf of up to 128 terms keeps eight running sums, the terms 8 apart, joined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail in order; above 128 terms pw(n) = pw(n2) + pw(n - n2) with
// n2 = n / 2 rounded down to a multiple of 8.  Lane j holds running sum j mod 8 (the lanes above 7 repeat the first eight, so every
// lane ends with the result); the recursion is an explicit stack, the same in every lane (12 levels: 128 * 2^12 terms).
template <class Term> __device__ double wave_np_pairwise_leaf(Term&& term, int off, int n, int lane) {
	if (n < 8) { double r = 0.0; for (int i = 0; i < n; ++i) r += term(off + i); return r; }
	const int j = lane & 7;
	double r = term(off + j);
	int i = 8;
	for (; i < n - (n % 8); i += 8) r += term(off + i + j);
	double q[8];
	for (int k = 0; k < 8; ++k) q[k] = __shfl(r, k, 64);
	double res = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
	for (; i < n; ++i) res += term(off + i);
	return res;
}
template <class Term> __device__ double wave_np_pairwise_sum(Term&& term, int n, int lane) {
	constexpr int kLevels = 12;
	int off[kLevels], len[kLevels], state[kLevels];
	double left[kLevels];
	int sp = 0;
	off[0] = 0; len[0] = n; state[0] = 0;
	double ret = 0.0;
	while (true) {
		int n2 = len[sp] / 2; n2 -= n2 % 8;
		if (state[sp] == 0) {
			if (len[sp] > 128 && sp < kLevels - 1) { state[sp] = 1; off[sp + 1] = off[sp]; len[sp + 1] = n2; state[sp + 1] = 0; ++sp; continue; }
			ret = wave_np_pairwise_leaf(term, off[sp], len[sp], lane);
		} else if (state[sp] == 1) {
			left[sp] = ret; state[sp] = 2; off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; state[sp + 1] = 0; ++sp; continue;
		} else ret = left[sp] + ret;
		if (sp == 0) break;
		--sp;
	}
	return ret;
}

// The same sum by ONE lane (halo_cubes.hip: the lanes of a wavefront are cadences, each with a sum of its own over the stamp): the
// leaf's eight running sums live in the lane's registers, the recursion is the same explicit stack (8 levels: 128 * 2^8 terms).
// n is the same in every lane, so the control flow is uniform.
template <class Term> __device__ double lane_np_pairwise_leaf(Term&& term, int off, int n) {
	if (n < 8) { double r = 0.0; for (int i = 0; i < n; ++i) r += term(off + i); return r; }
	double r[8];
#pragma unroll
	for (int j = 0; j < 8; ++j) r[j] = term(off + j);
	int i = 8;
	for (; i < n - (n % 8); i += 8) {
#pragma unroll
		for (int j = 0; j < 8; ++j) r[j] += term(off + i + j);
	}
	double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
	for (; i < n; ++i) res += term(off + i);
	return res;
}
template <class Term> __device__ double lane_np_pairwise_sum(Term&& term, int n) {
	constexpr int kLevels = 8;
	int off[kLevels], len[kLevels], state[kLevels];
	double left[kLevels];
	int sp = 0;
	off[0] = 0; len[0] = n; state[0] = 0;
	double ret = 0.0;
	while (true) {
		int n2 = len[sp] / 2; n2 -= n2 % 8;
		if (state[sp] == 0) {
			if (len[sp] > 128 && sp < kLevels - 1) { state[sp] = 1; off[sp + 1] = off[sp]; len[sp + 1] = n2; state[sp + 1] = 0; ++sp; continue; }
			ret = lane_np_pairwise_leaf(term, off[sp], len[sp]);
		} else if (state[sp] == 1) {
			left[sp] = ret; state[sp] = 2; off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; state[sp + 1] = 0; ++sp; continue;
		} else ret = left[sp] + ret;
		if (sp == 0) break;
		--sp;
	}
	return ret;
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

// how many threads before this one (in thread order) have the flag set, and how many of the block (`total`).  wcount: NT / 64 ints
// of LDS; the block synchronises before it calls again.
template <int NT> __device__ int block_rank(bool flag, int* wcount, int& total) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const unsigned long long b = __ballot(flag);
	if (lane == 0) wcount[wave] = __popcll(b);
	__syncthreads();
	int before = __popcll(b & ((1ull << lane) - 1ull));
	total = 0;
	for (int k = 0; k < NT / 64; k++) {
		if (k < wave) before += wcount[k];
		total += wcount[k];
	}
	return before;
}

struct Select {
	uint64_t key;
	int rank;   // how many equal keys precede the selected one in the order of the keys' owners (its occurrence index)
};

// The key of rank k (0-based, ascending) among the keys of the block: eight passes of eight bits (rules: RadixPass), a 256-bin
// integer histogram in LDS per pass, the bin picked by a scan over the first wave (four bins per lane).  each_key(visit) calls
// visit(key) for every key of this thread.  hist: 256 ints, sh: 2 ints of LDS.  Integer counts: exact whatever the order.
template <int NT, class Keys> __device__ __forceinline__ Select block_radix_select(Keys&& each_key, int k, int* hist, int* sh) {
	RadixPass pass = radix_begin(k);
	bool more = true;
	while (more) {
		for (int b = threadIdx.x; b < 256; b += NT) hist[b] = 0;
		__syncthreads();
		each_key([&](uint64_t key) { if (radix_takes_part(pass, key)) atomicAdd(&hist[radix_digit(pass, key)], 1); });
		__syncthreads();
		if (threadIdx.x < 64) {
			const int lane = threadIdx.x;
			const int c[4] = {hist[4 * lane], hist[4 * lane + 1], hist[4 * lane + 2], hist[4 * lane + 3]};
			const int s = c[0] + c[1] + c[2] + c[3];
			int inc = s;
			for (int o = 1; o < 64; o <<= 1) {
				const int v = __shfl_up(inc, o, 64);
				if (lane >= o) inc += v;
			}
			const int exc = inc - s;
			if (exc <= pass.krem && pass.krem < inc) {
				int b = 4 * lane, cum = exc;
				radix_walk(c, 4, pass.krem, b, cum);
				sh[0] = b;
				sh[1] = pass.krem - cum;
			}
		}
		__syncthreads();
		more = radix_next(pass, sh[0], sh[1]);
		__syncthreads();
	}
	return Select{pass.prefix, pass.krem};
}

// the device blocks of one host entry: handed out until one allocation fails (rc), freed when the entry returns
struct DevBlocks {
	tp_ctx* ctx;
	std::vector<void*> ptrs;
	int rc = TP_OK;
	explicit DevBlocks(tp_ctx* c) : ctx(c) {}
	template <class T> T* get(uint64_t count) {
		void* p = nullptr;
		if (rc == TP_OK) rc = tp_malloc(ctx, std::max<uint64_t>(count * sizeof(T), 16), &p);
		if (p) ptrs.push_back(p);
		return static_cast<T*>(p);
	}
	~DevBlocks() { for (void* p : ptrs) tp_free(ctx, p); }
};

} // namespace tp_halo
