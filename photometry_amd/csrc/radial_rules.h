// radial_rules.h -- what the radial ("corner glow") component of the full-frame background decides (radial.hip; evaluated where it is
// read: fullframe_dev.h), each rule stated once over plain values with the line of the reference it restates (backgrounds.py,
// utilities.py; statsmodels' bandwidths.py / kde.py / linbin.pyx / kdetools.py; scipy's scoreatpercentile; FITPACK's fpcurf / fpbspl /
// splev): the pixel and sample rules, the percentiles from selected order statistics, the ring mode (bandwidth, grid, linear binning,
// the FFT's butterfly, Silverman's factor, the argmax's grid value), the ring profile (moving median, knots, collocation rows, banded
// elimination) and the spline's evaluation, and the host checks of the entries.  No device code, no HIP runtime: the kernels call these
// from their parallel plumbing, tests/hostsim/radial_rules_host.cpp composes them serially under AddressSanitizer and UBSan, and
// tests/test_radial_rules_host.py holds that to the oracle and to scipy.
// (The build sets -ffp-contract=off: an expression gives the same bits here as written out in a kernel.)
#pragma once
#include <cmath>
#include <cstdint>
#include "select_rules.h"

// a short fixed-trip loop a kernel wants flat (a host compiler may do as it likes)
#if defined(__clang__)
#define TP_UNROLL _Pragma("unroll")
#else
#define TP_UNROLL
#endif

namespace tp_radial {

using tp_select::okey;
using tp_select::from_key;
using tp_select::RadixPass;
using tp_select::radix_begin;
using tp_select::radix_takes_part;
using tp_select::radix_digit;
using tp_select::radix_walk;
using tp_select::radix_next;

constexpr int kKdeGrid = 2048;       // statsmodels rounds gridsize = 2000 up to a power of two
constexpr int kKdeLog2 = 11;
constexpr int kMaxRings = 64;        // rings of a ring profile

//--------------------------------------------------------------------------------------------------
// pixels and samples
//--------------------------------------------------------------------------------------------------
// backgrounds.py:89-97 on the RAW image: NaN fails both comparisons
TP_RULE inline bool pixel_kept(float x, float flux_cutoff, bool excluded) { return (x >= 0.f) && (x <= flux_cutoff) && !excluded; }
// value = img - square: float32 before a square component exists (widened without loss), float64 after (:165)
TP_RULE inline double pixel_value(float x) { return (double)x; }
TP_RULE inline double pixel_value(float x, float square) { return (double)x - (double)square; }
// log10(img - square + zeropoint) (:168).  First round: numpy's float32 array + scalar stays float32, log10 of float32 (here the
// correctly rounded one); later rounds float64
TP_RULE inline double log_sample_first(double v, float zp32) { return (double)(float)log10((double)((float)v + zp32)); }
TP_RULE inline double log_sample(double v, double zp) { return log10(v + zp); }
// zeropoint = -min + 1.0 (:166-167, float64: numpy 1.21 promotes the float32 minimum of the first round); nothing unmasked
// (the minimum still +inf) -> NaN
TP_RULE inline double zeropoint_from_min(double mn) { return (mn == __builtin_inf()) ? __builtin_nan("") : (-mn + 1.0); }

//--------------------------------------------------------------------------------------------------
// selection and percentiles
//--------------------------------------------------------------------------------------------------
// the lower of the two order statistics (0-based) that scoreatpercentile(x, 100 frac) interpolates between; the median's lower one
TP_RULE inline int percentile_rank(int n, double frac) { return (int)(frac * (double)(n - 1)); }
TP_RULE inline int median_rank(int n) { return (n - 1) / 2; }
// the order statistic after rank k, whose value is v0: v0 again if more than k + 1 values are <= v0 (n_le), else the smallest larger
// value nxt (+inf: there is none, k is the last rank)
TP_RULE inline double next_order_statistic(double v0, int n_le, int k, double nxt) { return (n_le > k + 1 || nxt == __builtin_inf()) ? v0 : nxt; }
// scipy.stats.scoreatpercentile(x, per) (interpolation_method = 'fraction') from the two neighbouring order statistics
TP_RULE inline double percentile_from_pair(int n, double per, double s0, double s1)
{
	const double idx = per / 100.0 * (double)(n - 1);
	const int i = (int)idx;
	if ((double)i == idx) return s0;
	const double w0 = (double)(i + 1) - idx, w1 = idx - (double)i;
	return (s0 * w0 + s1 * w1) / (w0 + w1);
}
// np.median from the two middle order statistics
TP_RULE inline double median_from_pair(int n, double m0, double m1) { return (n & 1) ? m0 : 0.5 * (m0 + m1); }

//--------------------------------------------------------------------------------------------------
// the ring mode (_reduce_mode, backgrounds.py:20-32: KDEUnivariate.fit(gridsize = 2000), support[argmax(density)])
//--------------------------------------------------------------------------------------------------
// an empty ring is NaN (:21-22); one value gives a NaN bandwidth (std with ddof = 1), a NaN grid and support[0] = NaN; a NaN zero point
// (nothing unmasked in the frame) makes every sample NaN
TP_RULE inline bool ring_has_no_mode(int n, double zeropoint) { return n < 2 || !(zeropoint == zeropoint); }
TP_RULE inline double ring_mean(double sum, int n) { return sum / (double)n; }
// np.std(x, ddof = 1) from the sum of the squared deviations
TP_RULE inline double ring_std(double ss, int n) { return sqrt(ss / (double)(n - 1)); }
// bandwidths._select_sigma: min(std, IQR / 1.349), or std if IQR == 0
TP_RULE inline double ring_sigma(double sd, double q25, double q75)
{
	const double iqr = (q75 - q25) / 1.349;
	return (iqr > 0.0) ? fmin(sd, iqr) : sd;
}
// bandwidths.bw_normal_reference: C * A * n**(-1/5), C the kernel's normal-reference constant; 0 -> "Selected KDE bandwidth is 0":
// the ring's mode is its median (:27-31, median_from_pair)
TP_RULE inline double ring_bandwidth(double bw_constant, double sigma, int n) { return bw_constant * sigma * pow((double)n, -0.2); }

// kde.kdensityfft: the grid np.linspace(a, b, 2048) with a = min - cut * bw, b = max + cut * bw (cut = 3), RANGE = b - a
struct KdeGrid { double lo, hi, delta, range; };
TP_RULE inline KdeGrid kde_grid(double mn, double mx, double bw)
{
	KdeGrid g;
	g.lo = mn - 3.0 * bw;
	g.hi = mx + 3.0 * bw;
	g.delta = (g.hi - g.lo) / (double)(kKdeGrid - 1);
	g.range = g.hi - g.lo;
	return g;
}

// linbin.pyx fast_linbin with its "li > 1" guard: a sample gives 1 - rem to grid point li and rem to li + 1.  The two weights as
// 40-bit fixed-point integers (q and 2^40 - q: their sum is exact, and integer sums do not depend on the order of arrival); `lower` /
// `upper` say which of the two grid points exist
constexpr double kBinFix = 1099511627776.0;   // 2^40
struct BinPair { int li; bool lower, upper; unsigned long long w_lower, w_upper; };
TP_RULE inline BinPair bin_pair(double x, double lo, double delta)
{
	BinPair b;
	const double lx = (x - lo) / delta;
	b.li = (int)lx;
	const double rem = lx - (double)b.li;
	b.lower = b.li > 1 && b.li < kKdeGrid;
	b.upper = b.lower && b.li + 1 < kKdeGrid;
	const unsigned long long q = b.lower ? (unsigned long long)rint(rem * kBinFix) : 0ull;
	b.w_lower = (unsigned long long)kBinFix - q;
	b.w_upper = q;
	return b;
}
TP_RULE inline double bin_value(unsigned long long sum) { return (double)sum * (1.0 / kBinFix); }

// where grid point i stands before a decimation-in-time transform: its kKdeLog2 bits reversed
TP_RULE inline int bit_reversed(int i)
{
#if defined(__clang__)
	return (int)(__builtin_bitreverse32((unsigned)i) >> (32 - kKdeLog2));
#else
	unsigned r = 0;
	for (int b = 0; b < kKdeLog2; ++b) r |= (((unsigned)i >> b) & 1u) << (kKdeLog2 - 1 - b);
	return (int)r;
#endif
}
// butterfly b (0 .. 1023) of stage s (1 .. 11): the elements base and base + half, the twiddle exp(-2 pi i twiddle / 2048)
struct Butterfly { int base, half, twiddle; };
TP_RULE inline Butterfly butterfly_of(int s, int b)
{
	Butterfly f;
	f.half = 1 << (s - 1);
	const int j = b & (f.half - 1);
	f.base = ((b >> (s - 1)) << s) + j;
	f.twiddle = j * (kKdeGrid >> s);
	return f;
}
// (u, x) -> (u + w x, u - w x)
TP_RULE inline void butterfly(double wr, double wi, double& ur, double& ui, double& xr, double& xi)
{
	const double tr = xr * wr - xi * wi, ti = xr * wi + xi * wr;
	const double vr = ur, vi = ui;
	ur = vr + tr; ui = vi + ti;
	xr = vr - tr; xi = vi - ti;
}

// kdetools.silverman_transform: the Gaussian's transform at frequency J of 2048 (Hermitian: J and 2048 - J share a factor)
TP_RULE inline double silverman_fac1(double bw, double range) { return 2.0 * (M_PI * bw / range) * (M_PI * bw / range); }
TP_RULE inline double silverman_factor(int J, double fac1)
{
	const double jj = (double)((J <= kKdeGrid / 2) ? J : (kKdeGrid - J));
	const double t = jj / (double)kKdeGrid * M_PI;
	return exp(-(jj * jj) * fac1) / (1.0 - 1.0 / 3.0 * (t * t));
}
// np.linspace(lo, hi, 2048)[arg]: arange * step + lo, last point = hi
TP_RULE inline double grid_value(int arg, const KdeGrid& g) { return (arg == kKdeGrid - 1) ? g.hi : ((double)arg * g.delta + g.lo); }

//--------------------------------------------------------------------------------------------------
// the ring profile: utilities.move_median_central (utilities.py:52-62, backgrounds.py:178-179) and the interpolating cubic spline
// through the rings that have a mode (InterpolatedUnivariateSpline(k = 3), backgrounds.py:186: FITPACK puts its interior knots on the
// data points x[2 .. m-3] and solves the m x m collocation system)
//--------------------------------------------------------------------------------------------------
// np.nanmedian of up to 8 values
TP_RULE inline double nan_median(const double* v, int n)
{
	double w[8];
	int m = 0;
	for (int i = 0; i < n && i < 8; ++i) if (v[i] == v[i]) w[m++] = v[i];
	if (m == 0) return __builtin_nan("");
	for (int i = 1; i < m; ++i) { const double x = w[i]; int j = i; while (j > 0 && w[j - 1] > x) { w[j] = w[j - 1]; --j; } w[j] = x; }
	return (m & 1) ? w[m >> 1] : 0.5 * (w[(m >> 1) - 1] + w[m >> 1]);
}
// bottleneck.move_median(x, width, min_count = 1) at point i: the nan-median of the trailing window
TP_RULE inline double trailing_median(const double* x, int i, int width)
{
	const int a0 = (i - width + 1 > 0) ? (i - width + 1) : 0;
	return nan_median(x + a0, i + 1 - a0);
}
// np.roll(trail, -width // 2 + 1): Python floor division of the NEGATED width; point i of the rolled series is trail[rolled_index]
TP_RULE inline int roll_shift(int width) { return -((width + 1) / 2) + 1; }
TP_RULE inline int rolled_index(int i, int shift, int n) { return ((i - shift) % n + n) % n; }
// the ends redone over the first / last k + 2 points, k = 0 .. width / 2 (later ones overwrite earlier ones when the series is very
// short: in order)
TP_RULE inline void redo_ends(const double* x, int n, int width, double* prof)
{
	for (int k = 0; k < width / 2 + 1 && k < n; ++k) {
		const int c0 = (k + 2 < n) ? (k + 2) : n;
		prof[k] = nan_median(x, c0);
		prof[n - 1 - k] = nan_median(x + n - c0, c0);
	}
}
// fewer than 3 points: "The required number of points for qubic spline" (:183); exactly 3: FITPACK refuses (m > k); more knots than
// the caller's arrays hold: no radial component either
TP_RULE inline bool profile_has_no_spline(int m, int max_knots) { return m < 4 || m + 4 > max_knots; }
// knot i of the m + 4: the end points four times, between them the data points x[2 .. m-3] ("not a knot")
TP_RULE inline double knot_value(const double* x, int m, int i) { return (i < 4) ? x[0] : ((i < m) ? x[i - 2] : x[m - 1]); }
// collocation row i: the interval t[l] <= x[i] < t[l + 1] (the last point stays in the last interval) and the four cubic B-splines
// that are non-zero there, columns l - 3 .. l (fpbspl: de Boor's recurrence)
TP_RULE inline void collocation_row(const double* x, const double* t, int m, int i, int& l, double (&h)[4])
{
	l = 3;
	while (l < m - 1 && x[i] >= t[l + 1]) ++l;
	double hh[4];
	h[0] = 1.0; h[1] = 0.0; h[2] = 0.0; h[3] = 0.0;
	for (int j = 1; j <= 3; ++j) {
		for (int q = 0; q < j; ++q) hh[q] = h[q];
		h[0] = 0.0;
		for (int q = 0; q < j; ++q) {
			const int li = l + q + 1, lj = li - j;
			const double f = hh[q] / (t[li] - t[lj]);
			h[q] += f * (t[li] - x[i]);
			h[q + 1] = f * (x[i] - t[lj]);
		}
	}
}
// A row of the banded system is stored as 8 entries from a first column on.  Row i starts at the first column the elimination can
// still touch (i - 3 clipped); entry q of its collocation row (column l - 3 + q) goes to band_place, or nowhere (< 0)
TP_RULE inline int band_first_column(int i) { return (i - 3 > 0) ? (i - 3) : 0; }
TP_RULE inline int band_place(int l, int q, int first) { const int col = l - 3 + q - first; return (col >= 0 && col < 8) ? col : -1; }
// entry q of a row after moving its first column on by sh (left of the new first column it is already zero)
TP_RULE inline double rebased_entry(const double* row, int q, int sh) { return (sh > 0) ? ((q + sh < 8) ? row[q + sh] : 0.0) : row[q]; }
// partial pivoting inside the band: the largest |entry| of column c among rows c .. c + 3 (every row re-based to column c), the first
// of equals; no non-zero entry: row c itself
TP_RULE inline int pivot_row(const double (*A)[8], int c, int m)
{
	int piv = c;
	double best = 0.0;
	for (int k = c; k < m && k <= c + 3; ++k) {
		const double v = fabs(A[k][0]);
		if (v > best) { best = v; piv = k; }
	}
	return piv;
}
// one elimination update: row r loses f = a_r / d times the pivot row, entry by entry (and so does its right-hand side)
TP_RULE inline double elimination_factor(double a_r, double d) { return a_r / d; }
TP_RULE inline double eliminated(double v_r, double f, double v_c) { return v_r - f * v_c; }
// back substitution of row c (stored from column c on; after the exchanges it reaches at most column c + 6), y[c + 1 ..] solved
TP_RULE inline double back_substituted(const double (*A)[8], const double* y, int c, int m)
{
	const int rest = m - 1 - c;   // rows below c; `k <= rest` is `c + k < m`, asked this way (and the loops unrolled) one lane's chain of
	                              // m rows is 12 % shorter on the device than the parent's (profiles/radial_rules_refactor_time.txt)
	double ar[7], yr[7];
	TP_UNROLL
	for (int k = 0; k < 7; ++k) { ar[k] = A[c][k]; yr[k] = (k >= 1 && k <= rest) ? y[c + k] : 0.0; }
	double acc = y[c];
	TP_UNROLL
	for (int k = 1; k < 7; ++k) if (k <= rest) acc -= ar[k] * yr[k];
	return acc / ar[0];
}

//--------------------------------------------------------------------------------------------------
// the spline's evaluation: img_bkg_radial = 10**spline(r) - zeropoint (backgrounds.py:186-188; ext = 3: the boundary value outside
// the end knots) from the knots t[0..n), the coefficients c[0..n-4) and, per knot interval l, the six reciprocals of the knot
// differences de Boor's recursion divides by
//--------------------------------------------------------------------------------------------------
TP_RULE inline void knot_reciprocals(const double* t, int l, double* inv)
{
	inv[0] = 1.0 / (t[l + 3] - t[l]);
	inv[1] = 1.0 / (t[l + 2] - t[l - 1]);
	inv[2] = 1.0 / (t[l + 1] - t[l - 2]);
	inv[3] = 1.0 / (t[l + 2] - t[l]);
	inv[4] = 1.0 / (t[l + 1] - t[l - 1]);
	inv[5] = 1.0 / (t[l + 1] - t[l]);
}
// the spline at the distance of pixel (row, col) from the camera centre; n = the frame's number of knots (< 8: no radial component).
// inv: [l][6] (knot_reciprocals), filled for 3 <= l <= n - 5
TP_RULE inline double spline_at_pixel(const double* t, const double* c, const double* inv, int n, double col_offset, double xcen, double ycen, int row, int col)
{
	const double dx = ((double)col + col_offset) - xcen, dy = (double)row - ycen;
	double x = sqrt(dx * dx + dy * dy);
	x = fmin(fmax(x, t[3]), t[n - 4]);
	// interval t[l] <= x < t[l + 1], 3 <= l <= n - 5
	int l = 3, h = n - 4;
	while (h - l > 1) { const int m = (l + h) >> 1; if (x >= t[m]) l = m; else h = m; }
	const double* iv = inv + 6 * l;
	// de Boor, cubic
	double d0 = c[l - 3], d1 = c[l - 2], d2 = c[l - 1], d3 = c[l];
	double al;
	al = (x - t[l]) * iv[0];     d3 = (1.0 - al) * d2 + al * d3;
	al = (x - t[l - 1]) * iv[1]; d2 = (1.0 - al) * d1 + al * d2;
	al = (x - t[l - 2]) * iv[2]; d1 = (1.0 - al) * d0 + al * d1;
	al = (x - t[l]) * iv[3];     d3 = (1.0 - al) * d2 + al * d3;
	al = (x - t[l - 1]) * iv[4]; d2 = (1.0 - al) * d1 + al * d2;
	al = (x - t[l]) * iv[5];     d3 = (1.0 - al) * d2 + al * d3;
	return d3;
}
TP_RULE inline double radial_value(const double* t, const double* c, const double* inv, int n, double zeropoint, double col_offset, double xcen, double ycen,
	int row, int col)
{
	if (n < 8) return 0.0;
	return exp10(spline_at_pixel(t, c, inv, n, col_offset, xcen, ycen, row, col)) - zeropoint;
}

//--------------------------------------------------------------------------------------------------
// host checks of the entries
//--------------------------------------------------------------------------------------------------
inline bool radial_image_ok(int32_t n_frames, int64_t n_pixels, int64_t frame_stride)
{
	return n_frames >= 0 && n_frames <= 65535 && n_pixels > 0 && n_pixels <= 0x7fffffff && frame_stride >= n_pixels;
}
// (the spline indices are reflected once: the mesh must reach the last row and column of the frame it is evaluated on)
inline bool zoom_image_ok(bool have_arrays, int32_t mesh_rows, int32_t mesh_cols, int32_t box_size, int32_t frame_cols, int64_t n_pixels)
{
	return have_arrays && mesh_rows > 0 && mesh_cols > 0 && box_size > 0 && frame_cols > 0
		&& n_pixels % frame_cols == 0 && (int64_t)mesh_cols * box_size >= frame_cols
		&& (int64_t)mesh_rows * box_size >= n_pixels / frame_cols;
}
// an optional image beside the frames, dense [n_pixels]: one for all frames (stride 0) or one per frame
inline bool side_image_ok(bool have_image, int64_t stride, int64_t n_pixels) { return !have_image || stride == 0 || stride >= n_pixels; }

// The zero point's minimum with the square component evaluated from the mesh: threads walk down columns (col_blocks workgroups across
// a row), the rows divided into as many bands as the partial array holds -- if it holds a row of workgroups at all (a minimum does
// not depend on how the pixels are divided)
struct RowBands { int bands, rows_per_band; };
inline bool column_walk_fits(int col_blocks, int n_partial) { return col_blocks <= n_partial; }
inline RowBands row_bands(int n_rows, int n_partial, int col_blocks)
{
	RowBands b;
	b.bands = n_partial / col_blocks;
	if (b.bands > n_rows) b.bands = n_rows;
	b.rows_per_band = (n_rows + b.bands - 1) / b.bands;
	b.bands = (n_rows + b.rows_per_band - 1) / b.rows_per_band;
	return b;
}

} // namespace tp_radial
