// Host driver of the radial background's device-free rules (photometry_amd/csrc/radial_rules.h, select_rules.h), built with
// -fsanitize=address,undefined by tests/test_radial_rules_host.py.  It reads commands from stdin (tokens separated by white space;
// floating-point values travel as the hexadecimal bit pattern of the float32 / float64) and answers every command with lines on stdout:
//   keys N x1 .. xN                       -> N x "okey from_key(okey)"
//   select N K x1 .. xN k1 .. kK          -> K x "v0 v1": the serial radix selection of rank k and the next order statistic
//   percentiles N x1 .. xN                -> "q25 q50 q75 median": percentile_from_pair / median_from_pair on the selected pairs
//   pixel cutoff N, then N x (x excluded) -> N x 0 / 1 (x float32)
//   value N, then N x (x square)          -> N x "pixel_value(x) pixel_value(x, square)" (float32 in, float64 out)
//   logs zp N v1 .. vN                    -> N x "log_sample_first(v, float(zp)) log_sample(v, zp)"
//   zeropoint N mn1 .. mnN                -> N x zeropoint_from_min
//   mode C zp N x1 .. xN                  -> "n mode bw": the whole ring mode of the log samples x, composed serially
//   density C zp N x1 .. xN               -> the 2048 density values the mode is the argmax of (unnormalised; nothing if there is no grid)
//   median W N x1 .. xN                   -> N x the moving median of width W (move_median_central)
//   profile W max_knots N, then N x (bin_center mode) -> "n_knots", the knots, the coefficients
//   evaluate n t[n] c[n] zp col_offset xcen ycen P, then P x (row col) -> P x "float32(value) value"
//   imageok n_frames n_pixels stride | zoomok have rows cols box frame_cols n_pixels | sideok have stride n_pixels -> 0 / 1
//   bands n_rows n_partial col_blocks     -> "fits bands rows_per_band"
#include "radial_rules.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace tp_radial;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
uint64_t rd_hex() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return std::strtoull(s.c_str(), nullptr, 16); }
double rd_f64() { const uint64_t b = rd_hex(); double v; std::memcpy(&v, &b, 8); return v; }
float rd_f32() { const uint32_t b = (uint32_t)rd_hex(); float v; std::memcpy(&v, &b, 4); return v; }
uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
std::vector<double> rd_series(int64_t n) { std::vector<double> x((size_t)n); for (auto& v : x) v = rd_f64(); return x; }
void put(const std::vector<double>& a) { for (size_t i = 0; i < a.size(); i++) std::printf("%s%016" PRIx64, i ? " " : "", bits(a[i])); std::printf("\n"); }

// rank k and the order statistic after it: one histogram per pass, the bins walked serially; then the counts of the next-order rule
void select_pair(const std::vector<double>& x, int k, double& v0, double& v1) {
	RadixPass pass = radix_begin(k);
	for (bool more = true; more; ) {
		int hist[256] = {0};
		for (double v : x)
			if (radix_takes_part(pass, okey(v))) hist[radix_digit(pass, okey(v))]++;
		int b = 0, cum = 0;
		radix_walk(hist, 256, pass.krem, b, cum);
		more = radix_next(pass, b, pass.krem - cum);
	}
	v0 = from_key(pass.prefix);
	int n_le = 0;
	double nxt = INFINITY;
	for (double v : x) {
		n_le += (v <= v0) ? 1 : 0;
		if (v > v0) nxt = fmin(nxt, v);
	}
	v1 = next_order_statistic(v0, n_le, k, nxt);
}

// ---- the ring mode, the kernel's steps one after the other (sums in index order) ------------------------------------------------
void fft(std::vector<double>& re, std::vector<double>& im, const std::vector<double>& tw_re, const std::vector<double>& tw_im) {
	for (int s = 1; s <= kKdeLog2; s++)
		for (int b = 0; b < kKdeGrid / 2; b++) {
			const Butterfly f = butterfly_of(s, b);
			butterfly(tw_re[f.twiddle], tw_im[f.twiddle], re[f.base], im[f.base], re[f.base + f.half], im[f.base + f.half]);
		}
}

double ring_mode(const std::vector<double>& x, double bw_constant, double zp, double& bw, std::vector<double>* density = nullptr) {
	const int n = (int)x.size();
	bw = NAN;
	if (ring_has_no_mode(n, zp)) return NAN;
	double sum = 0.0, mn = INFINITY, mx = -INFINITY, ss = 0.0;
	for (double v : x) { sum += v; mn = fmin(mn, v); mx = fmax(mx, v); }
	const double mean = ring_mean(sum, n);
	for (double v : x) { const double d = v - mean; ss += d * d; }
	double a0, a1, b0, b1;
	select_pair(x, percentile_rank(n, 0.25), a0, a1);
	select_pair(x, percentile_rank(n, 0.75), b0, b1);
	const double sigma = ring_sigma(ring_std(ss, n), percentile_from_pair(n, 25.0, a0, a1), percentile_from_pair(n, 75.0, b0, b1));
	bw = ring_bandwidth(bw_constant, sigma, n);
	if (bw == 0.0) {
		double m0, m1;
		select_pair(x, median_rank(n), m0, m1);
		return median_from_pair(n, m0, m1);
	}
	const KdeGrid grid = kde_grid(mn, mx, bw);
	std::vector<unsigned long long> bins(kKdeGrid, 0ull);
	for (double v : x) {
		const BinPair b = bin_pair(v, grid.lo, grid.delta);
		if (b.lower) bins[bit_reversed(b.li)] += b.w_lower;
		if (b.upper) bins[bit_reversed(b.li + 1)] += b.w_upper;
	}
	std::vector<double> re(kKdeGrid), im(kKdeGrid, 0.0), tw_re(kKdeGrid / 2), tw_im(kKdeGrid / 2);
	for (int i = 0; i < kKdeGrid; i++) re[i] = bin_value(bins[i]);
	for (int i = 0; i < kKdeGrid / 2; i++) { tw_re[i] = cos(-2.0 * M_PI * (double)i / (double)kKdeGrid); tw_im[i] = sin(-2.0 * M_PI * (double)i / (double)kKdeGrid); }
	fft(re, im, tw_re, tw_im);
	const double fac1 = silverman_fac1(bw, grid.range);
	std::vector<double> zr(kKdeGrid), zi(kKdeGrid);
	for (int J = 0; J < kKdeGrid; J++) { const double fac = silverman_factor(J, fac1); zr[J] = re[J] * fac; zi[J] = -im[J] * fac; }
	for (int J = 0; J < kKdeGrid; J++) { re[bit_reversed(J)] = zr[J]; im[bit_reversed(J)] = zi[J]; }
	fft(re, im, tw_re, tw_im);
	if (density) *density = re;
	int arg = 0;
	for (int i = 1; i < kKdeGrid; i++) if (re[i] > re[arg]) arg = i;
	return grid_value(arg, grid);
}

// ---- the ring profile -------------------------------------------------------------------------------------------------------------
std::vector<double> moving_median(const std::vector<double>& s2, int width) {
	const int n = (int)s2.size();
	std::vector<double> prof(s2), trail((size_t)n);
	if (width > 1) {
		for (int i = 0; i < n; i++) trail[i] = trailing_median(s2.data(), i, width);
		for (int i = 0; i < n; i++) prof[i] = trail[rolled_index(i, roll_shift(width), n)];
		redo_ends(s2.data(), n, width, prof.data());
	}
	return prof;
}

// n_knots (0: no spline), knots t[0 .. m + 4), coefficients c[0 .. m)
int ring_profile(const std::vector<double>& bin_center, const std::vector<double>& s2, int width, int max_knots, std::vector<double>& t, std::vector<double>& c) {
	const std::vector<double> prof = moving_median(s2, width);
	std::vector<double> x, y;
	for (size_t i = 0; i < prof.size(); i++) if (prof[i] == prof[i]) { x.push_back(bin_center[i]); y.push_back(prof[i]); }
	const int m = (int)x.size();
	t.clear(); c.clear();
	if (profile_has_no_spline(m, max_knots)) return 0;
	for (int i = 0; i < m + 4; i++) t.push_back(knot_value(x.data(), m, i));
	std::vector<double> rows((size_t)m * 8, 0.0);
	double (*A)[8] = reinterpret_cast<double (*)[8]>(rows.data());
	std::vector<int> j0((size_t)m);
	for (int i = 0; i < m; i++) {
		int l;
		double h[4];
		collocation_row(x.data(), t.data(), m, i, l, h);
		j0[i] = band_first_column(i);
		for (int q = 0; q < 4; q++) { const int col = band_place(l, q, j0[i]); if (col >= 0) A[i][col] = h[q]; }
	}
	for (int col = 0; col < m; col++) {
		for (int r = col; r < m && r <= col + 3; r++) {
			double row[8];
			for (int q = 0; q < 8; q++) row[q] = rebased_entry(A[r], q, col - j0[r]);
			for (int q = 0; q < 8; q++) A[r][q] = row[q];
			j0[r] = col;
		}
		const int piv = pivot_row(A, col, m);
		if (piv != col) {
			for (int q = 0; q < 8; q++) std::swap(A[col][q], A[piv][q]);
			std::swap(y[col], y[piv]);
		}
		for (int r = col + 1; r < m && r <= col + 3; r++) {
			if (A[r][0] == 0.0) continue;
			const double f = elimination_factor(A[r][0], A[col][0]);
			for (int q = 0; q < 7; q++) A[r][q] = eliminated(A[r][q], f, A[col][q]);
			y[r] = eliminated(y[r], f, y[col]);
		}
	}
	for (int r = m - 1; r >= 0; r--) y[r] = back_substituted(A, y.data(), r, m);
	c = y;
	return m + 4;
}

void do_evaluate() {
	const int n = (int)rd();
	const std::vector<double> t = rd_series(n), c = rd_series(n);
	const double zp = rd_f64(), col_offset = rd_f64(), xcen = rd_f64(), ycen = rd_f64();
	std::vector<double> inv((size_t)6 * (n > 0 ? n : 1), 0.0);
	for (int l = 3; l <= n - 5; l++) knot_reciprocals(t.data(), l, inv.data() + 6 * l);
	for (int64_t p = rd(); p > 0; p--) {
		const int row = (int)rd(), col = (int)rd();
		const double v = radial_value(t.data(), c.data(), inv.data(), n, zp, col_offset, xcen, ycen, row, col);
		std::printf("%08" PRIx32 " %016" PRIx64 "\n", bits((float)v), bits(v));
	}
}

} // namespace

int main() {
	std::string cmd;
	while (std::cin >> cmd) {
		if (cmd == "keys") {
			for (double v : rd_series(rd())) std::printf("%016" PRIx64 " %016" PRIx64 "\n", okey(v), bits(from_key(okey(v))));
		} else if (cmd == "select") {
			const int64_t n = rd(), K = rd();
			const std::vector<double> x = rd_series(n);
			for (int64_t j = 0; j < K; j++) { double v0, v1; select_pair(x, (int)rd(), v0, v1); put({v0, v1}); }
		} else if (cmd == "percentiles") {
			const std::vector<double> x = rd_series(rd());
			const int n = (int)x.size();
			double a0, a1, b0, b1, c0, c1, m0, m1;
			select_pair(x, percentile_rank(n, 0.25), a0, a1);
			select_pair(x, percentile_rank(n, 0.5), b0, b1);
			select_pair(x, percentile_rank(n, 0.75), c0, c1);
			select_pair(x, median_rank(n), m0, m1);
			put({percentile_from_pair(n, 25.0, a0, a1), percentile_from_pair(n, 50.0, b0, b1), percentile_from_pair(n, 75.0, c0, c1), median_from_pair(n, m0, m1)});
		} else if (cmd == "pixel") {
			const float cutoff = rd_f32();
			for (int64_t n = rd(); n > 0; n--) { const float x = rd_f32(); const bool ex = rd() != 0; std::printf("%d\n", (int)pixel_kept(x, cutoff, ex)); }
		} else if (cmd == "value") {
			for (int64_t n = rd(); n > 0; n--) { const float x = rd_f32(), sq = rd_f32(); put({pixel_value(x), pixel_value(x, sq)}); }
		} else if (cmd == "logs") {
			const double zp = rd_f64();
			for (double v : rd_series(rd())) put({log_sample_first(v, (float)zp), log_sample(v, zp)});
		} else if (cmd == "zeropoint") {
			for (double v : rd_series(rd())) put({zeropoint_from_min(v)});
		} else if (cmd == "mode") {
			const double C = rd_f64(), zp = rd_f64();
			const std::vector<double> x = rd_series(rd());
			double bw;
			const double mode = ring_mode(x, C, zp, bw);
			std::printf("%d %016" PRIx64 " %016" PRIx64 "\n", (int)x.size(), bits(mode), bits(bw));
		} else if (cmd == "density") {
			const double C = rd_f64(), zp = rd_f64();
			const std::vector<double> x = rd_series(rd());
			double bw;
			std::vector<double> density;
			ring_mode(x, C, zp, bw, &density);
			put(density);
		} else if (cmd == "median") {
			const int width = (int)rd();
			put(moving_median(rd_series(rd()), width));
		} else if (cmd == "profile") {
			const int width = (int)rd(), max_knots = (int)rd();
			const int64_t n = rd();
			std::vector<double> bc, s2, t, c;
			for (int64_t i = 0; i < n; i++) { bc.push_back(rd_f64()); s2.push_back(rd_f64()); }
			std::printf("%d\n", ring_profile(bc, s2, width, max_knots, t, c));
			put(t);
			put(c);
		} else if (cmd == "evaluate") {
			do_evaluate();
		} else if (cmd == "imageok") {
			const int64_t a = rd(), b = rd(), c = rd();
			std::printf("%d\n", (int)radial_image_ok((int32_t)a, b, c));
		} else if (cmd == "zoomok") {
			const int64_t have = rd(), rows = rd(), cols = rd(), box = rd(), fc = rd(), np = rd();
			std::printf("%d\n", (int)zoom_image_ok(have != 0, (int32_t)rows, (int32_t)cols, (int32_t)box, (int32_t)fc, np));
		} else if (cmd == "sideok") {
			const int64_t have = rd(), stride = rd(), np = rd();
			std::printf("%d\n", (int)side_image_ok(have != 0, stride, np));
		} else if (cmd == "bands") {
			const int n_rows = (int)rd(), n_partial = (int)rd(), col_blocks = (int)rd();
			if (!column_walk_fits(col_blocks, n_partial)) { std::printf("0 0 0\n"); continue; }
			const RowBands b = row_bands(n_rows, n_partial, col_blocks);
			std::printf("1 %d %d\n", b.bands, b.rows_per_band);
		} else {
			std::printf("FAILED: unknown command %s\n", cmd.c_str());
			return 1;
		}
	}
	return 0;
}
