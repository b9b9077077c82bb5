// radial.hip -- the radial ("corner glow") component of backgrounds.fit_background for TESS full-frame images
// (photometry/backgrounds.py:104-197) on a frame stack resident in HBM.  Per iteration of its bkgiters loop:
//
//   tp_radial_zeropoint   zeropoint = -min(img - square over the unmasked pixels) + 1                       (:166-168)
//   tp_radial_ring_modes  per ring of 15 pixels beyond 2400 pixels from the camera centre: the mode of log10(img - square +
//                         zeropoint) -- argmax of statsmodels' FFT Gaussian KDE on 2048 grid points with the
//                         normal-reference bandwidth (_reduce_mode :20-32, binned_statistic :171-176)
//   tp_radial_profiles    3-point median of the ~40 ring modes and the interpolating cubic spline through them              (:179-187)
//   tp_radial_evaluate    img_bkg_radial = 10**spline(r) - zeropoint for every pixel (ext = 3: constant beyond the end knots), :188
//   The *_zoom entries take the square component (the previous iteration's zoomed mesh) as spline coefficients and evaluate it where
//   it is read (fullframe_dev.h): inside the alternation no frame-sized image is stored.
//
// What these kernels DECIDE -- every formula, threshold and index rule -- is stated once in radial_rules.h (device-free, held to the
// oracle on a CPU by tests/test_radial_rules_host.py); this file is the parallel plumbing, each kernel a sequence of named steps.
// The geometry (distance of every pixel from the camera centre, ring membership) does not depend on the frame: the host lists the
// pixels of every ring once (row-major inside a ring, like r[~mask] in the reference) and the ring kernel, one 256-thread workgroup
// per (ring, frame), walks its list: gather, spread, bandwidth, bin, density, mode.  It is bound by LDS and latency (18 passes over
// an L2-resident scratch row, two 2048-point FFTs); nothing in it depends on the order of arrival.
#include "common.h"
#include "fullframe_dev.h"
#include <cmath>

namespace {

using namespace tp_radial;   // the rules: radial_rules.h (and select_rules.h)

constexpr int kRadThreads = 256;
constexpr int kRadWaves = kRadThreads / 64;
constexpr int kRadBatch = 8;    // loads of the ring's scratch row in flight per thread

struct RadialImage {
	const float* frames; int64_t frame_stride;
	const float* square; int64_t square_stride;           // previous iteration's mesh background, or null (first iteration) ...
	bool zoom_on; ZoomImage zoom;                         // ... or the same image evaluated here from the mesh's spline coefficients
	const uint8_t* exclude; int64_t exclude_stride;       // manual-exclude image(s), stride 0 = shared
	float flux_cutoff;
};

// pixel_kept and pixel_value of pixel p, the square component read where it lies
// (x, excluded: the pixel's value and manual-exclude flag, loaded by the caller -- the ring kernel keeps several in flight)
__device__ __forceinline__ bool radial_pixel_loaded(const RadialImage& a, int frame, int64_t p, float x, bool excluded, double& value) {
	if (a.square) value = pixel_value(x, a.square[(int64_t)frame * a.square_stride + p]);
	else if (a.zoom_on) { const uint32_t q = (uint32_t)p, row = q / (uint32_t)a.zoom.n_cols;   // (pixel indices fit 31 bits: radial_image_ok)
		value = pixel_value(x, zoom_value(a.zoom, frame, (int)row, (int)(q - row * (uint32_t)a.zoom.n_cols))); }
	else value = pixel_value(x);
	return pixel_kept(x, a.flux_cutoff, excluded);
}
__device__ __forceinline__ bool radial_pixel(const RadialImage& a, int frame, int64_t p, double& value) {
	const float x = a.frames[(int64_t)frame * a.frame_stride + p];
	const bool excluded = a.exclude && a.exclude[(int64_t)frame * a.exclude_stride + p];
	return radial_pixel_loaded(a, frame, p, x, excluded, value);
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
	return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
	return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

// block-wide reductions through a 4-entry LDS array; every thread gets the result.  The four wavefronts' sums combine as
// (r0 + r1) + (r2 + r3): the order is part of the result's bits (halo_dev.h adds its partials one after the other -- not this one)
template <int OP>
__device__ __forceinline__ double block_reduce(double v, double* red) {
	static_assert(kRadWaves == 4, "four wavefront partials");
	v = (OP == 0) ? wave_sum(v) : (OP == 1) ? wave_min(v) : wave_max(v);
	__syncthreads();
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	if (OP == 0) return (red[0] + red[1]) + (red[2] + red[3]);
	if (OP == 1) return fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
	return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

__global__ __launch_bounds__(kRadThreads) void tp_radial_min_partial_kernel(RadialImage a, int64_t n_pix, double* __restrict__ partial)
{
	__shared__ double red[kRadWaves];
	const int frame = blockIdx.y;
	double mn = __builtin_inf();
	for (int64_t p = (int64_t)blockIdx.x * kRadThreads + threadIdx.x; p < n_pix; p += (int64_t)gridDim.x * kRadThreads) {
		double v;
		if (radial_pixel(a, frame, p, v)) mn = fmin(mn, v);
	}
	mn = block_reduce<1>(mn, red);
	if (threadIdx.x == 0) partial[(int64_t)frame * gridDim.x + blockIdx.x] = mn;
}

// The same with the square component evaluated from the mesh's spline coefficients: a thread walks down one column of a band of
// rows, so that the column's weights are formed once and the row sums of the coefficients once per mesh cell (zoom_sums).
// grid (column blocks, row bands, frames); partial [frame][gridDim.x * gridDim.y]
__global__ __launch_bounds__(kRadThreads) void tp_radial_min_zoom_kernel(RadialImage a, int n_rows, int n_cols, int rows_per_band, double* __restrict__ partial)
{
	__shared__ double red[kRadWaves];
	const int frame = blockIdx.z;
	const int col = blockIdx.x * kRadThreads + threadIdx.x;
	const int r0 = blockIdx.y * rows_per_band, r1 = (r0 + rows_per_band < n_rows) ? (r0 + rows_per_band) : n_rows;
	double mn = __builtin_inf();
	if (col < n_cols) {
		ZoomAxis ax, ay;
		zoom_axis(col, a.zoom.box, a.zoom.nx, ax);
		const double lo = a.zoom.vmin[frame], hi = a.zoom.vmax[frame];
		double T[4];
		int have = -0x7fffffff;
		for (int r = r0; r < r1; ++r) {
			const int64_t p = (int64_t)r * n_cols + col;
			const float x = a.frames[(int64_t)frame * a.frame_stride + p];
			const bool ok = pixel_kept(x, a.flux_cutoff, a.exclude && a.exclude[(int64_t)frame * a.exclude_stride + p]);
			zoom_axis(r, a.zoom.box, a.zoom.ny, ay);
			if (ay.start != have) { zoom_sums(a.zoom, frame, ay, ax, T); have = ay.start; }
			const double v = pixel_value(x, zoom_from_sums(ay, T, lo, hi));
			if (ok) mn = fmin(mn, v);
		}
	}
	mn = block_reduce<1>(mn, red);
	if (threadIdx.x == 0) partial[((int64_t)frame * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = mn;
}

// zeropoint_from_min of the partial minima
__global__ __launch_bounds__(kRadThreads) void tp_radial_min_final_kernel(const double* __restrict__ partial, int n_partial, double* __restrict__ zeropoint)
{
	__shared__ double red[kRadWaves];
	const int frame = blockIdx.x;
	double mn = __builtin_inf();
	for (int i = threadIdx.x; i < n_partial; i += kRadThreads) mn = fmin(mn, partial[(int64_t)frame * n_partial + i]);
	mn = block_reduce<1>(mn, red);
	if (threadIdx.x == 0) zeropoint[frame] = zeropoint_from_min(mn);
}

//--------------------------------------------------------------------------------------------------
// The ring kernel: one 256-thread workgroup per (ring, frame); the steps below in the order the kernel calls them
//--------------------------------------------------------------------------------------------------
struct RingArgs {
	RadialImage img;
	const double* zeropoint;
	const int32_t* ring_pixels; const int32_t* ring_offsets; int n_rings;
	double* scratch; int64_t scratch_stride;     // per frame: one row of ring_offsets[n_rings] float64
	double bw_constant;                          // the kernel's normal-reference constant 2 (1/24)^(1/5)
	double* modes; int32_t* counts;              // [frame][ring]
};

struct RingShared {
	double re[kKdeGrid], im[kKdeGrid];                     // the binned grid, its transform, the density
	double tw_re[kKdeGrid / 2], tw_im[kKdeGrid / 2];       // exp(-2 pi i k / 2048)
	double red[kRadWaves];                                 // block_reduce
	int hist[256];                                         // a radix pass's digit counts
	int wtot[kRadWaves];                                   // per-wavefront counts: kept pixels (gather), histogram totals (select_pair)
	int sh[2];                                             // the bin that holds the rank, the rank inside it
};

// the kept samples of a ring in its scratch row: their number and this thread's share of their sum, minimum and maximum
struct RingSamples { int n; double sum, mn, mx; };

// Walks the ring's scratch row vals[0..n) with kRadBatch loads in flight per thread and calls visit(value) for every element of this
// thread (i = tid, tid + 256, ...: ascending).  (The row lives in L2, and with one ring per workgroup and two or three workgroups per
// CU nothing else hides a load's latency -- a load per iteration was most of the ring kernel's time.)
template <class Visit>
__device__ __forceinline__ void walk_row(const double* __restrict__ vals, int n, Visit&& visit)
{
	for (int i0 = threadIdx.x; i0 < n; i0 += kRadBatch * kRadThreads) {
		double x[kRadBatch];
#pragma unroll
		for (int u = 0; u < kRadBatch; ++u) { const int i = i0 + u * kRadThreads; x[u] = vals[(i < n) ? i : (n - 1)]; }
#pragma unroll
		for (int u = 0; u < kRadBatch; ++u) if (i0 + u * kRadThreads < n) visit(x[u]);
	}
}

// The digit whose bin holds rank `rank`: the first d with hist[0] + ... + hist[d] > rank, into sh[0], and the rank inside the bin into
// sh[1] -- one bin per thread, an inclusive scan by shuffles inside the wavefronts and over their four totals (a single thread
// walking the 256 bins through LDS, radix_walk, was a seventh of the kernel's time: 16 such walks per ring)
__device__ __forceinline__ void bin_of_rank(int rank, RingShared& s)
{
	static_assert(kRadThreads == 256 && kRadWaves == 4, "one histogram bin per thread, four wavefront totals");
	const int tid = threadIdx.x;
	const int c = s.hist[tid];
	int x = c;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(x, off, 64); if ((tid & 63) >= off) x += y; }
	if ((tid & 63) == 63) s.wtot[tid >> 6] = x;
	__syncthreads();
	int before = 0;
	for (int w = 0; w < (tid >> 6); ++w) before += s.wtot[w];
	const int incl = x + before, excl = incl - c;
	if (excl <= rank && rank < incl) { s.sh[0] = tid; s.sh[1] = rank - excl; }
}

// k-th and (k+1)-th smallest of vals[0..n) (k + 1 clamped to n - 1): MSB-first radix selection, 8 bits per pass (select_rules.h)
__device__ void select_pair(const double* __restrict__ vals, int n, int k, RingShared& s, double& v0, double& v1)
{
	static_assert(kRadThreads == 256, "hist[tid] = 0 clears the 256 bins");
	const int tid = threadIdx.x;
	RadixPass pass = radix_begin(k);
	for (bool more = true; more; ) {
		s.hist[tid] = 0;
		__syncthreads();
		walk_row(vals, n, [&](double x) {
			const uint64_t key = okey(x);
			if (radix_takes_part(pass, key)) atomicAdd(&s.hist[radix_digit(pass, key)], 1);
		});
		__syncthreads();
		bin_of_rank(pass.krem, s);
		__syncthreads();
		more = radix_next(pass, s.sh[0], s.sh[1]);
		__syncthreads();
	}
	v0 = from_key(pass.prefix);
	int le = 0;
	double nxt = __builtin_inf();
	walk_row(vals, n, [&](double x) {
		le += (x <= v0) ? 1 : 0;
		if (x > v0) nxt = fmin(nxt, x);
	});
	const int n_le = (int)block_reduce<0>((double)le, s.red);
	nxt = block_reduce<1>(nxt, s.red);
	v1 = next_order_statistic(v0, n_le, k, nxt);
}

// ---- 1. gather, in the order of the ring's pixel list (row-major, like values[binnumber == j] in the reference): an ordered
// compaction -- per block of 256 list entries the kept ones are ranked by ballot / popcount inside a wavefront and by a four-entry
// count across the wavefronts.  Same order, same sums, same result in every run.
__device__ __forceinline__ RingSamples ring_gather(const RingArgs& a, int frame, int p0, int p1, double zp, double* vals, RingShared& s)
{
	static_assert(kRadThreads == 64 * kRadWaves, "one count per wavefront");
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const bool single = (a.img.square == nullptr) && !a.img.zoom_on;   // first iteration: float32 arithmetic
	const float zp32 = (float)zp;
	RingSamples g{0, 0.0, __builtin_inf(), -__builtin_inf()};
	for (int ib = p0; ib < p1; ib += kRadBatch * kRadThreads) {
		// the pixel indices, then the pixels, of the next kRadBatch steps: two dependent loads per step would otherwise be waited
		// for one step at a time
		int pix[kRadBatch];
		float xin[kRadBatch];
		bool exc[kRadBatch];
#pragma unroll
		for (int u = 0; u < kRadBatch; ++u) { const int i = ib + u * kRadThreads + tid; pix[u] = a.ring_pixels[(i < p1) ? i : (p1 - 1)]; }
#pragma unroll
		for (int u = 0; u < kRadBatch; ++u) {
			xin[u] = a.img.frames[(int64_t)frame * a.img.frame_stride + pix[u]];
			exc[u] = a.img.exclude && a.img.exclude[(int64_t)frame * a.img.exclude_stride + pix[u]];
		}
#pragma unroll
		for (int u = 0; u < kRadBatch; ++u) {
			const int i0 = ib + u * kRadThreads;
			if (i0 >= p1) break;                        // uniform
			double v = 0.0, lg = 0.0;
			const bool keep = (i0 + tid < p1) && radial_pixel_loaded(a.img, frame, pix[u], xin[u], exc[u], v);
			if (keep) lg = single ? log_sample_first(v, zp32) : log_sample(v, zp);
			const unsigned long long bal = __ballot(keep);
			if (lane == 0) s.wtot[wave] = __popcll(bal);
			__syncthreads();
			int before = 0, total = 0;
#pragma unroll
			for (int w = 0; w < kRadWaves; ++w) { const int c = s.wtot[w]; before += (w < wave) ? c : 0; total += c; }
			if (keep) {
				vals[g.n + before + __popcll(bal & ((1ull << lane) - 1ull))] = lg;
				g.sum += lg; g.mn = fmin(g.mn, lg); g.mx = fmax(g.mx, lg);
			}
			g.n += total;
			__syncthreads();
		}
	}
	return g;
}

// ---- 2. spread: the block's sum, minimum and maximum (into g), then std (two-pass, ddof = 1) and the quartiles by selection
struct RingSpread { double sd, q25, q75; };
__device__ __forceinline__ RingSpread ring_spread(const double* vals, RingSamples& g, RingShared& s)
{
	g.sum = block_reduce<0>(g.sum, s.red);
	g.mn = block_reduce<1>(g.mn, s.red);
	g.mx = block_reduce<2>(g.mx, s.red);
	__syncthreads();   // the scratch row is complete and visible
	const int n = g.n;
	const double mean = ring_mean(g.sum, n);
	double ss = 0.0;
	walk_row(vals, n, [&](double x) { const double d = x - mean; ss += d * d; });
	ss = block_reduce<0>(ss, s.red);
	double a0, a1, b0, b1;
	const int k25 = percentile_rank(n, 0.25), k75 = percentile_rank(n, 0.75);
	select_pair(vals, n, k25, s, a0, a1);
	select_pair(vals, n, k75, s, b0, b1);
	return RingSpread{ring_std(ss, n), percentile_from_pair(n, 25.0, a0, a1), percentile_from_pair(n, 75.0, b0, b1)};
}

// "Selected KDE bandwidth is 0" -> the median (:27-31)
__device__ __forceinline__ double ring_median(const double* vals, int n, RingShared& s)
{
	double m0, m1;
	select_pair(vals, n, median_rank(n), s, m0, m1);
	return median_from_pair(n, m0, m1);
}

// ---- 3. linear binning into s.re, bit-reversed for the decimation-in-time transform (and s.im = 0, the twiddles).  The weights are
// accumulated as 40-bit fixed-point integers with LDS integer atomics: the sum of integers does not depend on the order of arrival,
// so the binned grid is the same in every run (float atomics are not); the quantisation (2^-41 per sample) is far below the
// rounding of the float32 logarithm the samples come from.
__device__ __forceinline__ void ring_bin(const double* vals, int n, const KdeGrid& grid, RingShared& s)
{
	const int tid = threadIdx.x;
	unsigned long long* bins = reinterpret_cast<unsigned long long*>(s.re);
	for (int i = tid; i < kKdeGrid; i += kRadThreads) { bins[i] = 0ull; s.im[i] = 0.0; }
	for (int i = tid; i < kKdeGrid / 2; i += kRadThreads) {
		double sn, cs;
		sincospi(-2.0 * (double)i / (double)kKdeGrid, &sn, &cs);
		s.tw_re[i] = cs; s.tw_im[i] = sn;
	}
	__syncthreads();
	walk_row(vals, n, [&](double x) {
		const BinPair b = bin_pair(x, grid.lo, grid.delta);
		if (b.lower) atomicAdd(&bins[bit_reversed(b.li)], b.w_lower);
		if (b.upper) atomicAdd(&bins[bit_reversed(b.li + 1)], b.w_upper);
	});
	__syncthreads();
	for (int i = tid; i < kKdeGrid; i += kRadThreads) s.re[i] = bin_value(bins[i]);
	__syncthreads();
}

// one forward radix-2 transform of (re, im), in place, from bit-reversed to natural order
__device__ __forceinline__ void ring_fft(RingShared& s)
{
	for (int st = 1; st <= kKdeLog2; ++st) {
		for (int b = threadIdx.x; b < kKdeGrid / 2; b += kRadThreads) {
			const Butterfly f = butterfly_of(st, b);
			butterfly(s.tw_re[f.twiddle], s.tw_im[f.twiddle], s.re[f.base], s.im[f.base], s.re[f.base + f.half], s.im[f.base + f.half]);
		}
		__syncthreads();
	}
}

// ---- 4. density = IFFT(FFT(binned) * Silverman transform) into s.re; only its argmax is used (positive scale factors dropped).  The
// second forward transform of the conjugate is the inverse transform of a Hermitian spectrum.
__device__ __forceinline__ void ring_density(double bw, double range, RingShared& s)
{
	constexpr int kPer = kKdeGrid / kRadThreads;
	const int tid = threadIdx.x;
	const double fac1 = silverman_fac1(bw, range);
	ring_fft(s);
	// multiply by the kernel transform, conjugate, and put back in bit-reversed order for the second transform
	double zr[kPer], zi[kPer];
#pragma unroll
	for (int q = 0; q < kPer; ++q) {
		const int J = tid + q * kRadThreads;
		const double fac = silverman_factor(J, fac1);
		zr[q] = s.re[J] * fac; zi[q] = -s.im[J] * fac;
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < kPer; ++q) {
		const int r = bit_reversed(tid + q * kRadThreads);
		s.re[r] = zr[q]; s.im[r] = zi[q];
	}
	__syncthreads();
	ring_fft(s);
}

// ---- 5. mode: the first index of the density's maximum (np.argmax)
__device__ __forceinline__ int ring_argmax(RingShared& s)
{
	double best = -__builtin_inf();
	int best_i = kKdeGrid;
	for (int i = threadIdx.x; i < kKdeGrid; i += kRadThreads) {
		const double f = s.re[i];
		if (f > best) { best = f; best_i = i; }
	}
	const double wmax = block_reduce<2>(best, s.red);
	const int cand = (best == wmax) ? best_i : kKdeGrid;
	return (int)block_reduce<1>((double)cand, s.red);
}

__global__ __launch_bounds__(kRadThreads) void tp_radial_ring_kernel(RingArgs a)
{
	__shared__ RingShared s;
	const int ring = blockIdx.x, frame = blockIdx.y, tid = threadIdx.x;
	const int p0 = a.ring_offsets[ring], p1 = a.ring_offsets[ring + 1];
	double* vals = a.scratch + (int64_t)frame * a.scratch_stride + p0;
	const double zp = a.zeropoint[frame];
	double* mode_out = a.modes + (int64_t)frame * a.n_rings + ring;

	RingSamples g = ring_gather(a, frame, p0, p1, zp, vals, s);
	const int n = g.n;
	__threadfence_block();
	if (a.counts && tid == 0) a.counts[(int64_t)frame * a.n_rings + ring] = n;
	if (ring_has_no_mode(n, zp)) {
		if (tid == 0) *mode_out = __builtin_nan("");
		return;
	}
	const RingSpread sp = ring_spread(vals, g, s);
	const double bw = ring_bandwidth(a.bw_constant, ring_sigma(sp.sd, sp.q25, sp.q75), n);
	if (bw == 0.0) {
		const double med = ring_median(vals, n, s);
		if (tid == 0) *mode_out = med;
		return;
	}
	const KdeGrid grid = kde_grid(g.mn, g.mx, bw);
	ring_bin(vals, n, grid, s);
	ring_density(bw, grid.range, s);
	const int arg = ring_argmax(s);
	if (tid == 0) *mode_out = grid_value(arg, grid);
}

//--------------------------------------------------------------------------------------------------
// The ring profile of a frame: 3-point moving median of the ring modes and the interpolating cubic spline through the rings that
// have a mode (the rules: radial_rules.h).  A few dozen points per frame: one wavefront per frame, the collocation matrix (four
// non-zeros per row) in LDS.  One lane doing everything was a chain of ~3 000 LDS round trips (182 us per launch); the lanes share
// what is independent -- the moving medians, the collocation rows, and inside every pivot step of the elimination the (row, column)
// entries of the up to four rows it touches -- with every value formed by the same operations in the same order.
//--------------------------------------------------------------------------------------------------
struct ProfileShared {
	double A[kMaxRings][8];      // banded rows: columns j0 .. j0 + 7 of the row
	double s2l[kMaxRings], prof[kMaxRings], x[kMaxRings], y[kMaxRings], trail[kMaxRings], t[kMaxRings + 8];
	int j0[kMaxRings];
};

// ---- smooth: move_median_central of s.s2l[0..n) into s.prof
__device__ __forceinline__ void profile_smooth(int n, int width, ProfileShared& s)
{
	const int lane = threadIdx.x;
	if (width > 1) {
		if (lane < n) s.trail[lane] = trailing_median(s.s2l, lane, width);
		__syncthreads();
		if (lane < n) s.prof[lane] = s.trail[rolled_index(lane, roll_shift(width), n)];
		__syncthreads();
		if (lane == 0) redo_ends(s.s2l, n, width, s.prof);
	} else if (lane < n) {
		s.prof[lane] = s.s2l[lane];
	}
	__syncthreads();
}

// ---- compact: the rings that have a mode, in order, into (s.x, s.y); their number
__device__ __forceinline__ int profile_compact(const double* __restrict__ bin_center, int n, ProfileShared& s)
{
	const int lane = threadIdx.x;
	const bool has = (lane < n) && (s.prof[lane] == s.prof[lane]);
	const unsigned long long bal = __ballot(has);
	if (has) { const int pos = __popcll(bal & ((1ull << lane) - 1ull)); s.x[pos] = bin_center[lane]; s.y[pos] = s.prof[lane]; }
	__syncthreads();
	return __popcll(bal);
}

// ---- knots
__device__ __forceinline__ void profile_knots(int m, ProfileShared& s)
{
	for (int i = threadIdx.x; i < m + 4; i += 64) s.t[i] = knot_value(s.x, m, i);
	__syncthreads();
}

// ---- collocation rows: lane i builds row i, stored from band_first_column(i) on
__device__ __forceinline__ void profile_rows(int m, ProfileShared& s)
{
	const int lane = threadIdx.x;
	if (lane < m) {
		int l;
		double h[4];
		collocation_row(s.x, s.t, m, lane, l, h);
		const int first = band_first_column(lane);
		s.j0[lane] = first;
		for (int q = 0; q < 8; ++q) s.A[lane][q] = 0.0;
		for (int q = 0; q < 4; ++q) { const int col = band_place(l, q, first); if (col >= 0) s.A[lane][col] = h[q]; }
	}
	__syncthreads();
}

// ---- eliminate: Gaussian elimination with partial pivoting inside the band (row i has non-zeros in columns i - 3 .. i + 3 at most).
// Lane (rr, q) = (lane >> 3, lane & 7) of the first 32 holds entry q of row c + rr.
__device__ __forceinline__ void profile_eliminate(int m, ProfileShared& s)
{
	const int lane = threadIdx.x, rr = lane >> 3, q = lane & 7;
	for (int c = 0; c < m; ++c) {
		const int r = c + rr;
		const bool mine = (rr < 4) && (r < m);
		// the rows that can have an entry in column c are c .. c + 3: re-base them to c
		double val = 0.0;
		if (mine) val = rebased_entry(s.A[r], q, c - s.j0[r]);
		__syncthreads();
		if (mine) { s.A[r][q] = val; if (q == 0) s.j0[r] = c; }
		__syncthreads();
		const int piv = pivot_row(s.A, c, m);
		if (piv != c) {      // (uniform: every lane found the same pivot)
			double u0 = 0.0, u1 = 0.0;
			if (rr == 0) { u0 = s.A[c][q]; u1 = s.A[piv][q]; }
			__syncthreads();
			if (rr == 0) { s.A[c][q] = u1; s.A[piv][q] = u0; }
			if (lane == 0) { const double ty = s.y[c]; s.y[c] = s.y[piv]; s.y[piv] = ty; }
			__syncthreads();
		}
		const double d = s.A[c][0];
		double neu = 0.0, f = 0.0;
		bool upd = false;
		if (mine && rr >= 1) {
			const double a0 = s.A[r][0];
			if (a0 != 0.0) {
				upd = true;
				f = elimination_factor(a0, d);
				if (q < 7) neu = eliminated(s.A[r][q], f, s.A[c][q]);   // after the exchanges a row reaches at most column c + 6
			}
		}
		__syncthreads();
		if (upd) {
			if (q < 7) s.A[r][q] = neu;
			else s.y[r] = eliminated(s.y[r], f, s.y[c]);
		}
		__syncthreads();
	}
}

// ---- back-substitute: the coefficients into s.y, last row first
__device__ __forceinline__ void profile_back_substitute(int m, ProfileShared& s)
{
	if (threadIdx.x == 0)
		for (int c = m - 1; c >= 0; --c) s.y[c] = back_substituted(s.A, s.y, c, m);
	__syncthreads();
}

__global__ __launch_bounds__(64) void tp_radial_profile_kernel(const double* __restrict__ modes, const double* __restrict__ bin_center, int n_rings,
	int width, int n_frames, int max_knots, double* __restrict__ knots, double* __restrict__ coefs, int32_t* __restrict__ n_knots)
{
	__shared__ ProfileShared s;
	const int frame = blockIdx.x, lane = threadIdx.x;
	if (frame >= n_frames) return;
	if (lane < n_rings) s.s2l[lane] = modes[(int64_t)frame * n_rings + lane];
	__syncthreads();
	profile_smooth(n_rings, width, s);
	const int m = profile_compact(bin_center, n_rings, s);
	if (profile_has_no_spline(m, max_knots)) { if (lane == 0) n_knots[frame] = 0; return; }
	profile_knots(m, s);
	profile_rows(m, s);
	profile_eliminate(m, s);
	profile_back_substitute(m, s);
	// ---- store
	double* kt = knots + (int64_t)frame * max_knots;
	double* kc = coefs + (int64_t)frame * max_knots;
	for (int i = lane; i < m + 4; i += 64) kt[i] = s.t[i];
	for (int i = lane; i < m; i += 64) kc[i] = s.y[i];
	if (lane == 0) n_knots[frame] = m + 4;
}

struct EvalArgs {
	int n_rows, n_cols; int64_t frame_stride;
	RadialSpline sp;
	const float* add; int64_t add_stride;
	bool zoom_on; ZoomImage zoom;         // the square component evaluated here instead of read from `add`
	float* out;
};

// out = float32(10**spline(r) - zeropoint [+ add]); a frame with n_knots == 0 has no radial component (out = add or 0).
// A workgroup takes 256 columns of a strip of kEvalRows rows; a thread walks down its column (the square component from the mesh
// coefficients: column weights once, row sums once per mesh cell).
constexpr int kEvalRows = 16;
__global__ __launch_bounds__(256) void tp_radial_eval_kernel(EvalArgs a)
{
	extern __shared__ double sp[];   // knots, coefficients, reciprocal knot differences (stage_radial)
	const int frame = blockIdx.z;
	const int n = a.sp.n_knots[frame];
	stage_radial(sp, a.sp.max_knots, a.sp, frame, n, threadIdx.x, 256);
	const int col = blockIdx.x * 256 + threadIdx.x;
	if (col >= a.n_cols) return;
	const int r0 = blockIdx.y * kEvalRows, r1 = (r0 + kEvalRows < a.n_rows) ? (r0 + kEvalRows) : a.n_rows;
	const double zp = a.sp.zeropoint[frame];
	ZoomAxis ax, ay;
	double T[4], lo = 0.0, hi = 0.0;
	int have = -0x7fffffff;
	if (a.zoom_on) { zoom_axis(col, a.zoom.box, a.zoom.nx, ax); lo = a.zoom.vmin[frame]; hi = a.zoom.vmax[frame]; }
	for (int row = r0; row < r1; ++row) {
		const int64_t p = (int64_t)row * a.n_cols + col;
		const double radial = radial_value(sp, a.sp.max_knots, n, zp, a.sp.col_offset, a.sp.xcen, a.sp.ycen, row, col);
		double base = 0.0;
		if (a.add) base = (double)a.add[(int64_t)frame * a.add_stride + p];
		else if (a.zoom_on) {
			zoom_axis(row, a.zoom.box, a.zoom.ny, ay);
			if (ay.start != have) { zoom_sums(a.zoom, frame, ay, ax, T); have = ay.start; }
			base = (double)zoom_from_sums(ay, T, lo, hi);
		}
		a.out[(int64_t)frame * a.frame_stride + p] = (float)(radial + base);
	}
}

} // namespace

// the host checks of the entries: radial_rules.h
static bool zoom_image_ok(const tp_zoom_image* z, int64_t n_pixels) {
	return z && tp_radial::zoom_image_ok(z->d_coef && z->d_vmin && z->d_vmax, z->mesh_rows, z->mesh_cols, z->box_size, z->frame_cols, n_pixels);
}
static bool side_image_ok(const void* d_image, int64_t stride, int64_t n_pixels) { return tp_radial::side_image_ok(d_image != nullptr, stride, n_pixels); }
static ZoomImage zoom_of(const tp_zoom_image* z) {
	return ZoomImage{z->d_coef, z->d_vmin, z->d_vmax, z->mesh_rows, z->mesh_cols, z->box_size, z->frame_cols};
}

static int radial_zeropoint_launch(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const float* d_square, int64_t square_frame_stride, const tp_zoom_image* zoom, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	double* d_partial, int32_t n_partial, double* d_zeropoint)
{
	TP_REQUIRE(ctx, d_frames && d_partial && d_zeropoint, "tp_radial_zeropoint: null pointer");
	TP_REQUIRE(ctx, radial_image_ok(n_frames, n_pixels, frame_stride), "tp_radial_zeropoint: bad frame geometry");
	TP_REQUIRE(ctx, n_partial >= 1 && n_partial <= 65535, "tp_radial_zeropoint: n_partial must be 1..65535");
	TP_REQUIRE(ctx, zoom == nullptr || (zoom_image_ok(zoom, n_pixels) && d_square == nullptr), "tp_radial_zeropoint_zoom: bad mesh image");
	TP_REQUIRE(ctx, side_image_ok(d_square, square_frame_stride, n_pixels), "tp_radial_zeropoint: square_frame_stride must be 0 or at least n_pixels");
	TP_REQUIRE(ctx, side_image_ok(d_exclude, exclude_frame_stride, n_pixels), "tp_radial_zeropoint: exclude_frame_stride must be 0 or at least n_pixels");
	if (n_frames == 0) return TP_OK;
	RadialImage img{d_frames, frame_stride, d_square, square_frame_stride, zoom != nullptr, zoom ? zoom_of(zoom) : ZoomImage{}, d_exclude, exclude_frame_stride, (float)flux_cutoff};
	int n_used = n_partial;
	const int n_cols = zoom ? zoom->frame_cols : 0;
	const int col_blocks = zoom ? (n_cols + kRadThreads - 1) / kRadThreads : 0;
	if (zoom && column_walk_fits(col_blocks, n_partial)) {
		const int n_rows = (int)(n_pixels / n_cols);
		const RowBands b = row_bands(n_rows, n_partial, col_blocks);
		n_used = b.bands * col_blocks;
		TP_LAUNCH(ctx, TPK_BKG_RADIAL, tp_radial_min_zoom_kernel, dim3((unsigned)col_blocks, (unsigned)b.bands, (unsigned)n_frames), dim3(kRadThreads), 0,
			img, n_rows, n_cols, b.rows_per_band, d_partial);
	} else {
		TP_LAUNCH(ctx, TPK_BKG_RADIAL, tp_radial_min_partial_kernel, dim3((unsigned)n_partial, (unsigned)n_frames), dim3(kRadThreads), 0, img, n_pixels, d_partial);
	}
	TP_LAUNCH(ctx, TPK_BKG_RADIAL, tp_radial_min_final_kernel, dim3((unsigned)n_frames), dim3(kRadThreads), 0, d_partial, n_used, d_zeropoint);
	TP_LAUNCH_CHECK(ctx, "tp_radial_min kernels");
	return TP_OK;
}

extern "C" int tp_radial_zeropoint(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const float* d_square, int64_t square_frame_stride, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	double* d_partial, int32_t n_partial, double* d_zeropoint)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	return radial_zeropoint_launch(ctx, d_frames, n_frames, n_pixels, frame_stride, d_square, square_frame_stride, nullptr, d_exclude, exclude_frame_stride,
		flux_cutoff, d_partial, n_partial, d_zeropoint);
	TP_API_END(ctx)
}

extern "C" int tp_radial_zeropoint_zoom(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const tp_zoom_image* square, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	double* d_partial, int32_t n_partial, double* d_zeropoint)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, square != nullptr, "tp_radial_zeropoint_zoom: null mesh image");
	return radial_zeropoint_launch(ctx, d_frames, n_frames, n_pixels, frame_stride, nullptr, 0, square, d_exclude, exclude_frame_stride,
		flux_cutoff, d_partial, n_partial, d_zeropoint);
	TP_API_END(ctx)
}

static int radial_ring_launch(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const float* d_square, int64_t square_frame_stride, const tp_zoom_image* zoom, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	const double* d_zeropoint, const int32_t* d_ring_pixels, const int32_t* d_ring_offsets, int32_t n_rings, int32_t n_ring_pixels,
	double bandwidth_constant, double* d_scratch, double* d_modes, int32_t* d_counts)
{
	TP_REQUIRE(ctx, d_frames && d_zeropoint && d_ring_pixels && d_ring_offsets && d_scratch && d_modes, "tp_radial_ring_modes: null pointer");
	TP_REQUIRE(ctx, radial_image_ok(n_frames, n_pixels, frame_stride), "tp_radial_ring_modes: bad frame geometry");
	TP_REQUIRE(ctx, n_rings >= 0 && n_rings <= 65535 && n_ring_pixels >= 0, "tp_radial_ring_modes: bad ring list");
	TP_REQUIRE(ctx, zoom == nullptr || (zoom_image_ok(zoom, n_pixels) && d_square == nullptr), "tp_radial_ring_modes_zoom: bad mesh image");
	TP_REQUIRE(ctx, side_image_ok(d_square, square_frame_stride, n_pixels), "tp_radial_ring_modes: square_frame_stride must be 0 or at least n_pixels");
	TP_REQUIRE(ctx, side_image_ok(d_exclude, exclude_frame_stride, n_pixels), "tp_radial_ring_modes: exclude_frame_stride must be 0 or at least n_pixels");
	if (n_frames == 0 || n_rings == 0) return TP_OK;
	RingArgs a;
	a.img = RadialImage{d_frames, frame_stride, d_square, square_frame_stride, zoom != nullptr, zoom ? zoom_of(zoom) : ZoomImage{}, d_exclude, exclude_frame_stride, (float)flux_cutoff};
	a.zeropoint = d_zeropoint;
	a.ring_pixels = d_ring_pixels; a.ring_offsets = d_ring_offsets; a.n_rings = n_rings;
	a.scratch = d_scratch; a.scratch_stride = n_ring_pixels;
	a.bw_constant = bandwidth_constant;
	a.modes = d_modes; a.counts = d_counts;
	TP_LAUNCH(ctx, TPK_BKG_RADIAL, tp_radial_ring_kernel, dim3((unsigned)n_rings, (unsigned)n_frames), dim3(kRadThreads), 0, a);
	TP_LAUNCH_CHECK(ctx, "tp_radial_ring_kernel");
	return TP_OK;
}

extern "C" int tp_radial_ring_modes(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const float* d_square, int64_t square_frame_stride, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	const double* d_zeropoint, const int32_t* d_ring_pixels, const int32_t* d_ring_offsets, int32_t n_rings, int32_t n_ring_pixels,
	double bandwidth_constant, double* d_scratch, double* d_modes, int32_t* d_counts)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	return radial_ring_launch(ctx, d_frames, n_frames, n_pixels, frame_stride, d_square, square_frame_stride, nullptr, d_exclude, exclude_frame_stride, flux_cutoff,
		d_zeropoint, d_ring_pixels, d_ring_offsets, n_rings, n_ring_pixels, bandwidth_constant, d_scratch, d_modes, d_counts);
	TP_API_END(ctx)
}

extern "C" int tp_radial_ring_modes_zoom(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const tp_zoom_image* square, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	const double* d_zeropoint, const int32_t* d_ring_pixels, const int32_t* d_ring_offsets, int32_t n_rings, int32_t n_ring_pixels,
	double bandwidth_constant, double* d_scratch, double* d_modes, int32_t* d_counts)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, square != nullptr, "tp_radial_ring_modes_zoom: null mesh image");
	return radial_ring_launch(ctx, d_frames, n_frames, n_pixels, frame_stride, nullptr, 0, square, d_exclude, exclude_frame_stride, flux_cutoff,
		d_zeropoint, d_ring_pixels, d_ring_offsets, n_rings, n_ring_pixels, bandwidth_constant, d_scratch, d_modes, d_counts);
	TP_API_END(ctx)
}

static int radial_evaluate_launch(tp_ctx* ctx, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	double col_offset, double xcen, double ycen, const double* d_knots, const double* d_coefs, const int32_t* d_n_knots, int32_t max_knots,
	const double* d_zeropoint, const float* d_add, int64_t add_frame_stride, const tp_zoom_image* zoom, float* d_out)
{
	TP_REQUIRE(ctx, d_knots && d_coefs && d_n_knots && d_zeropoint && d_out, "tp_radial_evaluate: null pointer");
	TP_REQUIRE(ctx, n_frames >= 0 && n_frames <= 65535 && frame_rows > 0 && frame_rows <= 65535 && frame_cols > 0
		&& frame_stride >= (int64_t)frame_rows * frame_cols, "tp_radial_evaluate: bad frame geometry");
	TP_REQUIRE(ctx, max_knots >= 8 && max_knots <= 1024, "tp_radial_evaluate: max_knots must be 8..1024");
	TP_REQUIRE(ctx, zoom == nullptr || (zoom_image_ok(zoom, (int64_t)frame_rows * frame_cols) && d_add == nullptr && zoom->frame_cols == frame_cols), "tp_radial_evaluate_zoom: bad mesh image");
	TP_REQUIRE(ctx, side_image_ok(d_add, add_frame_stride, (int64_t)frame_rows * frame_cols), "tp_radial_evaluate: add_frame_stride must be 0 or at least frame_rows * frame_cols");
	if (n_frames == 0) return TP_OK;
	EvalArgs a;
	a.n_rows = frame_rows; a.n_cols = frame_cols; a.frame_stride = frame_stride;
	a.sp = RadialSpline{col_offset, xcen, ycen, d_knots, d_coefs, d_n_knots, max_knots, d_zeropoint};
	a.add = d_add; a.add_stride = add_frame_stride;
	a.zoom_on = zoom != nullptr; a.zoom = zoom ? zoom_of(zoom) : ZoomImage{};
	a.out = d_out;
	dim3 grid((unsigned)((frame_cols + 255) / 256), (unsigned)((frame_rows + kEvalRows - 1) / kEvalRows), (unsigned)n_frames);
	TP_LAUNCH(ctx, TPK_BKG_RADIAL, tp_radial_eval_kernel, grid, dim3(256), (size_t)kRadialStageDoubles(max_knots) * sizeof(double), a);
	TP_LAUNCH_CHECK(ctx, "tp_radial_eval_kernel");
	return TP_OK;
}

extern "C" int tp_radial_evaluate(tp_ctx* ctx, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	double col_offset, double xcen, double ycen, const double* d_knots, const double* d_coefs, const int32_t* d_n_knots, int32_t max_knots,
	const double* d_zeropoint, const float* d_add, int64_t add_frame_stride, float* d_out)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	return radial_evaluate_launch(ctx, n_frames, frame_rows, frame_cols, frame_stride, col_offset, xcen, ycen, d_knots, d_coefs, d_n_knots, max_knots,
		d_zeropoint, d_add, add_frame_stride, nullptr, d_out);
	TP_API_END(ctx)
}

extern "C" int tp_radial_evaluate_zoom(tp_ctx* ctx, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	const tp_radial_image* radial, const tp_zoom_image* add, float* d_out)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, radial != nullptr && add != nullptr, "tp_radial_evaluate_zoom: null ring profile / mesh image");
	return radial_evaluate_launch(ctx, n_frames, frame_rows, frame_cols, frame_stride, radial->col_offset, radial->xcen, radial->ycen,
		radial->d_knots, radial->d_coefs, radial->d_n_knots, radial->max_knots, radial->d_zeropoint, nullptr, 0, add, d_out);
	TP_API_END(ctx)
}

extern "C" int tp_radial_profiles(tp_ctx* ctx, int32_t n_frames, int32_t n_rings, const double* d_modes, const double* d_bin_center,
	int32_t radial_smooth, int32_t max_knots, double* d_knots, double* d_coefs, int32_t* d_n_knots)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, d_modes && d_bin_center && d_knots && d_coefs && d_n_knots, "tp_radial_profiles: null pointer");
	TP_REQUIRE(ctx, n_frames >= 0 && n_rings >= 1 && n_rings <= kMaxRings, "tp_radial_profiles: at most 64 rings");
	TP_REQUIRE(ctx, radial_smooth >= 0 && radial_smooth <= 8 && max_knots >= n_rings + 4, "tp_radial_profiles: radial_smooth must be 0..8, max_knots >= n_rings + 4");
	if (n_frames == 0) return TP_OK;
	TP_LAUNCH(ctx, TPK_BKG_RADIAL, tp_radial_profile_kernel, dim3((unsigned)n_frames), dim3(64), 0, d_modes, d_bin_center, (int)n_rings,
		(int)radial_smooth, (int)n_frames, (int)max_knots, d_knots, d_coefs, d_n_knots);
	TP_LAUNCH_CHECK(ctx, "tp_radial_profile_kernel");
	return TP_OK;
	TP_API_END(ctx)
}
