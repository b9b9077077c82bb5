// Host driver of Halo photometry's device-free rules (photometry_amd/csrc/halo_rules.h), built with -fsanitize=address,undefined by
// tests/test_halo_rules_host.py.  It reads commands from stdin (tokens separated by white space; floating-point values travel as the
// hexadecimal bit pattern of the float32 / float64) and answers every command with lines on stdout:
//   keys N x1 .. xN                      -> N x "okey from_key(okey)" (float64)
//   fkeys N x1 .. xN                     -> N x "fkey from_fkey(fkey)" (float32)
//   select N K x1 .. xN k1 .. kK         -> K x "value occurrence": the serial radix selection composed from the pass rules
//   median N x1 .. xN                    -> the median from the middle ranks and their keys
//   drop minflux M, then M x (n x1 .. xn float32) -> M x 0 / 1: drop_pixel on the counts the select kernel gathers
//   finite N x1 .. xN (float32)          -> N x 0 / 1
//   offset g[9] st[4] N p1 .. pN         -> N x stamp_offset
//   solver n rows history align (d_P as an address), then rows x (p_off npix ncad), then rows x status (-1: none given)
//                                        -> "check MSG", "limit MSG", per problem the 10 fields of HaloProb, "totals ..", "plist ..", "list2 .."
//   settings maxiter history ftol gtol   -> 0 / 1
//   poll objective maxiter N             -> max_steps and the first N poll counts
//   seglists T n_seg bitmask, then T x (seg quality) -> cadlist, fitlist, seg_off, tiles
//   stack g[9] have_stack n_stamps, stamps, have_seg, seg[T] -> "stack MSG", "seg MSG" (MSG "ok" for none)
//   gather g[9] n_run, then n_run x (index p_off npix ncad) -> "MSG max_ncad", then per problem the 6 fields
//   norm g[9] n_run, then n_run x (index npix ncad)         -> "MSG", then per problem the 5 fields, then "run .."
//   machine nf maxiter history ftol gtol objective N, then N events "s ft valid" | "f gmax sy yy gtd gtd_steepest"
//                                        -> the state after init and after every event
//   lbfgs npix ncad maxiter history ftol gtol, fit bytes, P float32 [ncad][npix]
//                                        -> "status iterations f", then w: the whole optimiser, transitions from the header
#include "halo_rules.h"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

using namespace tp_halo;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
uint64_t rd_hex() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return std::strtoull(s.c_str(), nullptr, 16); }
double rd_f64() { const uint64_t b = rd_hex(); double v; std::memcpy(&v, &b, 8); return v; }
float rd_f32() { const uint32_t b = (uint32_t)rd_hex(); float v; std::memcpy(&v, &b, 4); return v; }
uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
StackGeom rd_geom() { StackGeom g; int32_t* f = &g.n_frames; for (int k = 0; k < 9; k++) f[k] = (int32_t)rd(); return g; }
template <class T> void line(const char* name, const std::vector<T>& a) { std::printf("%s", name); for (auto v : a) std::printf(" %" PRId64, (int64_t)v); std::printf("\n"); }

// the key of rank k among x, and how many equal values precede the selected one: one histogram per pass, the bins walked serially
void serial_select(const std::vector<double>& x, int k, uint64_t& key, int& occurrence) {
	RadixPass pass = radix_begin(k);
	bool more = true;
	while (more) {
		int hist[256] = {0};
		for (double v : x)
			if (radix_takes_part(pass, okey(v))) hist[radix_digit(pass, okey(v))]++;
		int b = 0, cum = 0;
		radix_walk(hist, 256, pass.krem, b, cum);
		more = radix_next(pass, b, pass.krem - cum);
	}
	key = pass.prefix;
	occurrence = pass.krem;
}
// the index of the occurrence-th value with that key, in the order of x
int find_occurrence(const std::vector<double>& x, uint64_t key, int occurrence) {
	for (size_t j = 0; j < x.size(); j++)
		if (okey(x[j]) == key && occurrence-- == 0) return (int)j;
	return -1;
}

// ---- the optimiser, serially -----------------------------------------------------------------------------------------------
struct Machine {
	HaloState s;
	int maxiter, H, objective;
	double ftol, gtol;
};

int stat_step(Machine& M, double ft, double m, bool valid, int t0, int t1) {
	const HaloState st = M.s;
	const int outcome = stat_decide(st, ft, valid);
	if (outcome == kStatAccept) stat_accept(M.s, st, ft, m, t0, t1);
	else if (outcome == kStatDegenerate) stat_degenerate(M.s);
	else if (outcome == kStatLineSearchFailed) stat_line_search_failed(M.s, st);
	else stat_next_trial(M.s, st, next_alpha(st));
	return outcome;
}

// the finish step as tp_halo_finish_kernel walks it; `num` supplies the numbers: gradient() -> |g|_inf, first_gradient(),
// pair_products(alpha, sy, yy), move_on(alpha, keep, slot, sy, yy), two_loop(n_pairs, newest) -> g.d, steepest() -> g.d, first_trial()
template <class Numbers> void finish_step(Machine& M, Numbers& num) {
	const HaloState st = M.s;
	if (st.status != ST_ACTIVE || !st.need_grad) return;
	const double gmax = num.gradient(st);
	int status, n_pairs = st.n_pairs, newest = st.newest;
	if (st.initial) {
		if (M.objective) { finish_objective(M.s); return; }
		num.first_gradient();
		status = stop_initial(gmax, M.gtol, M.maxiter);
	} else {
		double sy, yy;
		num.pair_products(st.alpha, sy, yy);
		const bool keep = pair_kept(sy, yy);
		const int slot = next_slot(newest, M.H);
		num.move_on(st.alpha, keep, slot, sy, yy);
		if (keep) pair_stored(slot, M.H, n_pairs, newest);
		status = stop_step(st.f_prev, st.f, gmax, st.iters, M.ftol, M.gtol, M.maxiter);
	}
	if (status != ST_ACTIVE) { finish_stopped(M.s, status, n_pairs, newest); return; }
	double gtd = 0.0;
	if (n_pairs > 0) {
		gtd = num.two_loop(n_pairs, newest);
		if (!is_descent(gtd)) n_pairs = 0;
	}
	if (n_pairs == 0) gtd = num.steepest();
	num.first_trial();
	finish_next_search(M.s, gtd, n_pairs, newest);
}

void print_state(const char* what, const Machine& M) {
	const HaloState& s = M.s;
	std::printf("%s %d %d %d %d %d %d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " slots", what, s.status, s.iters, s.trials, s.need_grad,
		s.initial, s.n_pairs, s.newest, bits(s.alpha), bits(s.f), bits(s.f_prev), bits(s.gtd));
	for (int i = 0; i < s.n_pairs; i++) std::printf(" %d", pair_slot(s.newest, s.n_pairs, i, M.H));
	std::printf("\n");
}

// the numbers of a finish step read from the script
struct Scripted {
	double gmax, sy, yy, gtd, gtd_steepest;
	double gradient(const HaloState&) { return gmax; }
	void first_gradient() {}
	void pair_products(double, double& a, double& b) { a = sy; b = yy; }
	void move_on(double, bool, int, double, double) {}
	double two_loop(int, int) { return gtd; }
	double steepest() { return gtd_steepest; }
	void first_trial() {}
};

void do_machine() {
	Machine M;
	const int nf = (int)rd();
	M.maxiter = (int)rd(); M.H = (int)rd(); M.ftol = rd_f64(); M.gtol = rd_f64(); M.objective = (int)rd();
	state_init(M.s, nf);
	print_state("init", M);
	for (int64_t n = rd(); n > 0; n--) {
		std::string kind;
		std::cin >> kind;
		if (kind == "s") {
			const double ft = rd_f64();
			const bool valid = rd() != 0;
			if (M.s.status == ST_ACTIVE) stat_step(M, ft, 1.0, valid, 0, 0);
			print_state("stat", M);
		} else {
			Scripted num;
			num.gmax = rd_f64(); num.sy = rd_f64(); num.yy = rd_f64(); num.gtd = rd_f64(); num.gtd_steepest = rd_f64();
			finish_step(M, num);
			print_state("finish", M);
		}
	}
}

// the numbers of a real problem: plain serial sums
struct Problem {
	int npix, ncad, H;
	std::vector<float> P;
	std::vector<int> fidx;
	std::vector<double> theta, g, d, w, q, l, S, Y, ssy, syy, sgn;
	double at(int j) const { return l[fidx[j]]; }

	void softmax(double alpha, bool with_d) {
		double mx = -INFINITY;
		for (int p = 0; p < npix; p++) mx = fmax(mx, with_d ? theta[p] + alpha * d[p] : theta[p]);
		double s = 0.0;
		for (int p = 0; p < npix; p++) { w[p] = exp((with_d ? theta[p] + alpha * d[p] : theta[p]) - mx); s += w[p]; }
		for (int p = 0; p < npix; p++) w[p] = w[p] / s;
	}
	void forward() {
		for (int t = 0; t < ncad; t++) {
			double acc = 0.0;
			for (int p = 0; p < npix; p++) acc += w[p] * (double)P[(size_t)t * npix + p];
			l[t] = acc;
		}
	}
	// the stat step: TV, sign terms, median and its cadences
	int stat(Machine& M) {
		const int nf = (int)fidx.size();
		double tv = 0.0;
		std::vector<double> lF(nf);
		for (int j = 0; j < nf; j++) {
			lF[j] = at(j);
			const double dp = j > 0 ? at(j) - at(j - 1) : 0.0, dn = j + 1 < nf ? at(j + 1) - at(j) : 0.0;
			sgn[fidx[j]] = (double)sign_term(dp, dn);
			tv += fabs(dn);
		}
		const int k1 = mid_lo(nf), k2 = mid_hi(nf);
		uint64_t key1, key2;
		int occ1, occ2;
		serial_select(lF, k1, key1, occ1);
		serial_select(lF, k2, key2, occ2);
		const double m = median_of_keys(key1, key2, k2 != k1);
		const bool valid = median_valid(m);
		return stat_step(M, objective_value(tv, m, valid), m, valid, fidx[find_occurrence(lF, key1, occ1)], fidx[find_occurrence(lF, key2, occ2)]);
	}
	double gradient(const HaloState& st) {
		const int ntiles = (ncad + kTile - 1) / kTile;
		const double m = st.m, fm = st.f / m;
		const float* r0 = P.data() + (size_t)st.tmed0 * npix;
		const float* r1 = P.data() + (size_t)st.tmed1 * npix;
		double wg = 0.0;
		for (int p = 0; p < npix; p++) {
			const double G = sum_tiles(ntiles, [&](int tile) {
				double acc = 0.0;
				for (int t = tile * kTile; t < std::min((tile + 1) * kTile, ncad); t++)
					if (sgn[t] != 0.0) acc += sgn[t] * (double)P[(size_t)t * npix + p];
				return acc;
			});
			q[p] = grad_w(G, m, fm, median_row(r0, r1, st.tmed0 == st.tmed1, p));
			wg += w[p] * q[p];
		}
		double gmax = 0.0;
		for (int p = 0; p < npix; p++) { q[p] = w[p] * (q[p] - wg); gmax = fmax(gmax, fabs(q[p])); }
		return gmax;
	}
	void first_gradient() { g = q; }
	void pair_products(double alpha, double& sy, double& yy) {
		sy = yy = 0.0;
		for (int p = 0; p < npix; p++) {
			const double tn = theta[p] + alpha * d[p];
			const double s = tn - theta[p], y = q[p] - g[p];
			sy += s * y;
			yy += y * y;
		}
	}
	void move_on(double alpha, bool keep, int slot, double sy, double yy) {
		for (int p = 0; p < npix; p++) {
			const double tn = theta[p] + alpha * d[p];
			if (keep) { S[(size_t)slot * npix + p] = tn - theta[p]; Y[(size_t)slot * npix + p] = q[p] - g[p]; }
			theta[p] = tn;
			g[p] = q[p];
		}
		if (keep) { ssy[slot] = sy; syy[slot] = yy; }
	}
	double dot(const double* a, const double* b) const { double v = 0.0; for (int p = 0; p < npix; p++) v += a[p] * b[p]; return v; }
	double two_loop(int n_pairs, int newest) {
		std::vector<double> sa(n_pairs);
		d = g;
		for (int i = n_pairs - 1; i >= 0; i--) {
			const int k = pair_slot(newest, n_pairs, i, H);
			sa[i] = (1.0 / ssy[k]) * dot(&S[(size_t)k * npix], d.data());
			for (int p = 0; p < npix; p++) d[p] -= sa[i] * Y[(size_t)k * npix + p];
		}
		const double gamma = gamma_of(ssy[newest], syy[newest]);
		for (int p = 0; p < npix; p++) d[p] = gamma * d[p];
		for (int i = 0; i < n_pairs; i++) {
			const int k = pair_slot(newest, n_pairs, i, H);
			const double b = (1.0 / ssy[k]) * dot(&Y[(size_t)k * npix], d.data());
			for (int p = 0; p < npix; p++) d[p] += S[(size_t)k * npix + p] * (sa[i] - b);
		}
		for (int p = 0; p < npix; p++) d[p] = -d[p];
		return dot(g.data(), d.data());
	}
	double steepest() {
		const double nrm = sqrt(dot(g.data(), g.data()));
		for (int p = 0; p < npix; p++) d[p] = -g[p] / nrm;
		return dot(g.data(), d.data());
	}
	void first_trial() { softmax(1.0, true); }
};

void do_lbfgs() {
	Problem pb;
	Machine M;
	pb.npix = (int)rd(); pb.ncad = (int)rd();
	M.maxiter = (int)rd(); M.H = pb.H = (int)rd(); M.ftol = rd_f64(); M.gtol = rd_f64(); M.objective = 0;
	for (int t = 0; t < pb.ncad; t++)
		if (rd()) pb.fidx.push_back(t);
	pb.P.resize((size_t)pb.ncad * pb.npix);
	for (auto& v : pb.P) v = rd_f32();
	for (auto* a : {&pb.theta, &pb.g, &pb.d, &pb.w, &pb.q}) a->assign(pb.npix, 0.0);
	pb.l.assign(pb.ncad, 0.0); pb.sgn.assign(pb.ncad, 0.0);
	pb.S.assign((size_t)pb.H * pb.npix, 0.0); pb.Y = pb.S;
	pb.ssy.assign(pb.H, 0.0); pb.syy = pb.ssy;
	state_init(M.s, (int)pb.fidx.size());
	pb.softmax(0.0, false);
	const int64_t limit = max_steps(0, M.maxiter);
	for (int64_t step = 0; step < limit && M.s.status == ST_ACTIVE; step++) {
		pb.forward();
		if (pb.stat(M) == kStatNextTrial) pb.softmax(M.s.alpha, true);
		finish_step(M, pb);
	}
	pb.softmax(0.0, false);
	std::printf("%d %d %016" PRIx64 "\n", M.s.status, M.s.iters, bits(M.s.status == ST_DEGENERATE ? (double)NAN : M.s.f));
	for (double v : pb.w) std::printf("%016" PRIx64 " ", bits(v));
	std::printf("\n");
}

// ---- tables ------------------------------------------------------------------------------------------------------------------
void do_solver() {
	const int32_t n = (int32_t)rd(), rows = (int32_t)rd(), history = (int32_t)rd();
	const uintptr_t align = (uintptr_t)rd();
	std::vector<int64_t> off(rows); std::vector<int32_t> npix(off.size()), ncad(off.size());
	for (size_t i = 0; i < off.size(); i++) { off[i] = rd(); npix[i] = (int32_t)rd(); ncad[i] = (int32_t)rd(); }
	std::vector<HaloState> states(off.size());
	bool given = true;
	for (auto& s : states) { s.status = (int32_t)rd(); given = given && s.status >= 0; }
	const char* bad = solver_check(n, off.data(), npix.data(), ncad.data(), reinterpret_cast<const void*>(align), &n);
	std::printf("check %s\n", bad ? bad : "ok");
	if (bad || n == 0) return;
	const SolverLayout L = solver_layout(n, off.data(), npix.data(), ncad.data(), history);
	bad = solver_layout_check(L);
	std::printf("limit %s\n", bad ? bad : "ok");
	if (bad || L.tiles_tot > (1 << 20)) return;   // (the lists of a batch at the limit are not printed)
	for (const HaloProb& p : L.prob)
		std::printf("prob %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d %d %d\n", p.p_off, p.c_off, p.w_off, p.o_off, p.h_off, p.part_off, p.npix,
			p.pitch, p.ncad, p.ntiles);
	std::printf("totals %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d\n", L.c_tot, L.w_tot, L.o_tot, L.part_tot, L.tiles_tot, L.max_pitch);
	std::vector<int32_t> list2, plist;
	launch_lists(L.prob, given ? states.data() : nullptr, list2, plist);
	line("plist", plist);
	line("list2", list2);
}

void do_seglists() {
	const int32_t T = (int32_t)rd(), n_seg = (int32_t)rd(), bitmask = (int32_t)rd();
	std::vector<int32_t> seg(T), quality(T);
	for (int t = 0; t < T; t++) { seg[t] = (int32_t)rd(); quality[t] = (int32_t)rd(); }
	const SegLists s = seg_lists(T, n_seg, seg.data(), quality.data(), bitmask);
	line("cadlist", s.cadlist); line("fitlist", s.fitlist); line("seg_off", s.seg_off); line("tiles", s.tiles);
}

void do_stack() {
	const StackGeom g = rd_geom();
	const bool have_stack = rd() != 0;
	std::vector<int32_t> stamps((size_t)rd() * 4);
	for (auto& v : stamps) v = (int32_t)rd();
	const bool have_seg = rd() != 0;
	std::vector<int32_t> seg(have_seg ? std::max(g.n_frames, 0) : 0);
	for (auto& v : seg) v = (int32_t)rd();
	const char* bad = stack_check(g, have_stack ? &g : nullptr, stamps.empty() ? nullptr : stamps.data());
	std::printf("stack %s\n", bad ? bad : "ok");
	bad = seg_check(g, have_seg ? seg.data() : nullptr);
	std::printf("seg %s\n", bad ? bad : "ok");
}

void do_gather() {
	const StackGeom g = rd_geom();
	const int32_t n = (int32_t)rd();
	std::vector<int32_t> index(n), npix(n), ncad(n); std::vector<int64_t> off(n);
	for (int r = 0; r < n; r++) { index[r] = (int32_t)rd(); off[r] = rd(); npix[r] = (int32_t)rd(); ncad[r] = (int32_t)rd(); }
	std::vector<GatherProb> probs;
	int32_t max_ncad = 0;
	const char* bad = gather_table(g, n, index.data(), off.data(), npix.data(), ncad.data(), probs, max_ncad);
	std::printf("%s\n", bad ? bad : "ok");
	if (bad) return;
	std::printf("max_ncad %d\n", max_ncad);
	for (const GatherProb& p : probs) std::printf("prob %" PRId64 " %" PRId64 " %d %d %d %d\n", p.p_off, p.c_off, p.q, p.npix, p.ncad, p.pitch);
}

void do_norm() {
	const StackGeom g = rd_geom();
	const int32_t n = (int32_t)rd();
	std::vector<int32_t> index(n), npix(n), ncad(n);
	for (int r = 0; r < n; r++) { index[r] = (int32_t)rd(); npix[r] = (int32_t)rd(); ncad[r] = (int32_t)rd(); }
	std::vector<NormProb> probs;
	std::vector<int32_t> run;
	const char* bad = norm_table(g, n, index.data(), npix.data(), ncad.data(), probs, run);
	std::printf("%s\n", bad ? bad : "ok");
	if (bad) return;
	for (const NormProb& p : probs) std::printf("prob %" PRId64 " %" PRId64 " %d %d %d\n", p.c_off, p.w_off, p.q, p.npix, p.ncad);
	line("run", run);
}

void do_drop() {
	const double minflux = rd_f64();
	for (int64_t m = rd(); m > 0; m--) {
		// the counts as tp_halo_select_stat_kernel gathers them
		int32_t n = 0, c = 0;
		uint32_t ak = 0u, bk = 0xffffffffu;
		for (int64_t k = rd(); k > 0; k--) {
			const float x = rd_f32();
			if (x != x) continue;
			n++;
			if ((double)x < minflux) { c++; ak = std::max(ak, fkey(x)); }
			else bk = std::min(bk, fkey(x));
		}
		std::printf("%d ", (int)drop_pixel(n, c, ak, bk, minflux));
	}
	std::printf("\n");
}

std::vector<double> rd_series(int64_t n) { std::vector<double> x((size_t)n); for (auto& v : x) v = rd_f64(); return x; }

void do_select() {
	const int64_t n = rd(), K = rd();
	const std::vector<double> x = rd_series(n);
	for (int64_t i = 0; i < K; i++) {
		uint64_t key; int occ;
		serial_select(x, (int)rd(), key, occ);
		std::printf("%016" PRIx64 " %d\n", bits(from_key(key)), occ);
	}
}

void do_median() {
	const std::vector<double> x = rd_series(rd());
	const int nf = (int)x.size();
	uint64_t lo, hi; int occ;
	serial_select(x, mid_lo(nf), lo, occ);
	serial_select(x, mid_hi(nf), hi, occ);
	std::printf("%016" PRIx64 "\n", bits(median_of_keys(lo, hi, mid_hi(nf) != mid_lo(nf))));
}

} // namespace

int main() {
	std::string cmd;
	while (std::cin >> cmd) {
		if (cmd == "keys") {
			for (double v : rd_series(rd())) std::printf("%016" PRIx64 " %016" PRIx64 "\n", okey(v), bits(from_key(okey(v))));
		} else if (cmd == "fkeys") {
			for (int64_t n = rd(); n > 0; n--) { const float v = rd_f32(); std::printf("%08" PRIx32 " %08" PRIx32 "\n", fkey(v), bits(from_fkey(fkey(v)))); }
		} else if (cmd == "select") {
			do_select();
		} else if (cmd == "median") {
			do_median();
		} else if (cmd == "drop") {
			do_drop();
		} else if (cmd == "finite") {
			for (int64_t n = rd(); n > 0; n--) std::printf("%d ", (int)pixel_finite(rd_f32()));
			std::printf("\n");
		} else if (cmd == "offset") {
			const StackGeom g = rd_geom();
			int32_t st[4];
			for (auto& v : st) v = (int32_t)rd();
			for (int64_t n = rd(); n > 0; n--) std::printf("%" PRId64 " ", stamp_offset(g, st, (int)rd()));
			std::printf("\n");
		} else if (cmd == "solver") {
			do_solver();
		} else if (cmd == "settings") {
			const int32_t maxiter = (int32_t)rd(), history = (int32_t)rd();
			const double ftol = rd_f64(), gtol = rd_f64();
			std::printf("%d\n", (int)settings_ok(maxiter, history, ftol, gtol));
		} else if (cmd == "poll") {
			const int objective = (int)rd();
			const int32_t maxiter = (int32_t)rd();
			std::printf("%" PRId64, max_steps(objective, maxiter));
			int32_t poll = first_poll(objective);
			for (int64_t n = rd(); n > 0; n--, poll = next_poll(poll)) std::printf(" %d", poll);
			std::printf("\n");
		} else if (cmd == "seglists") {
			do_seglists();
		} else if (cmd == "stack") {
			do_stack();
		} else if (cmd == "gather") {
			do_gather();
		} else if (cmd == "norm") {
			do_norm();
		} else if (cmd == "machine") {
			do_machine();
		} else if (cmd == "lbfgs") {
			do_lbfgs();
		} else { std::printf("FAILED: unknown command '%s'\n", cmd.c_str()); return 2; }
	}
	return 0;
}
