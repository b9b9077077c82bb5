// Host driver of the frames engine's device-free rules (photometry_amd/csrc/frames_rules.h), built with -fsanitize=address,undefined by
// tests/test_frames_rules_host.py.  It reads commands from stdin (tokens separated by white space; floating-point values travel as the
// hexadecimal bit pattern of the float32 / float64) and answers every command with lines on stdout:
//   size_class K n1 .. nK                               -> the K size classes
//   pairwise N x1 .. xN                                 -> the bits of np_pairwise_sum
//   catalog N, then N x (starid tmag row col)           -> (nothing: builds the index the `select` commands use)
//   select M K, then M x (r1 r2 c1 c2)                  -> the selection of the M stamps, made in K runs joined by append: 7 lines
//                                                          (cat_offsets, starid, tmag, row, col, row_stamp, col_stamp)
//   block m T H W cap                                   -> the 8 offsets of BlockLayout and nbytes
//   meta T m n_cat                                      -> the 14 offsets of MetaLayout and nbytes
//   plan T cubes budget N, then N x (r1 r2 c1 c2)       -> "parts P", then per part "part Q" and Q x "piece H W nbytes n idx.."
//   decide flags status stamp[4] limits[4] attempts budget H W, then H*W mask bytes, H*W sum-image values
//                                                       -> outcome status moved stamp[4] kind edge_flux n_codes codes..
#include "frames_rules.h"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

namespace fr = frames_rules;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
uint64_t rd_hex() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return std::strtoull(s.c_str(), nullptr, 16); }
double rd_f64() { const uint64_t b = rd_hex(); double v; std::memcpy(&v, &b, 8); return v; }
float rd_f32() { const uint32_t b = (uint32_t)rd_hex(); float v; std::memcpy(&v, &b, 4); return v; }
uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

void line(const std::vector<int64_t>& a) { for (int64_t v : a) std::printf("%" PRId64 " ", v); std::printf("\n"); }
void line(const std::vector<float>& a) { for (float v : a) std::printf("%08" PRIx32 " ", bits(v)); std::printf("\n"); }

std::vector<int64_t> rd_stamps(int64_t n) { std::vector<int64_t> st((size_t)n * 4); for (auto& v : st) v = rd(); return st; }

void do_select(const fr::CatalogIndex& index) {
	const int64_t m = rd(), K = rd();
	const std::vector<int64_t> st = rd_stamps(m);
	std::vector<int32_t> idx((size_t)m);
	for (int64_t j = 0; j < m; ++j) idx[(size_t)j] = (int32_t)j;
	fr::Selection all;
	for (int64_t k = 0; k < K; ++k) {
		const size_t a = (size_t)(m * k / K), b = (size_t)(m * (k + 1) / K);
		all.append(fr::select_catalog(index, st.data(), idx.data() + a, b - a));
	}
	line(all.cat_offsets); line(all.starid); line(all.tmag); line(all.row); line(all.col); line(all.row_stamp); line(all.col_stamp);
}

void do_plan() {
	const int32_t T = (int32_t)rd();
	const bool cubes = rd() != 0;
	const double budget = rd_f64();
	const int64_t n = rd();
	const std::vector<int64_t> st = rd_stamps(n);
	std::vector<int32_t> active;
	for (int64_t i = 0; i < n; ++i) active.push_back((int32_t)i);
	const auto parts = fr::plan_round(active, st.data(), T, cubes, budget);
	std::printf("parts %zu\n", parts.size());
	for (const auto& part : parts) {
		std::printf("part %zu\n", part.size());
		for (const fr::Piece& p : part) {
			std::printf("piece %d %d %016" PRIx64 " %zu", p.H, p.W, bits(p.nbytes), p.idx.size());
			for (int32_t i : p.idx) std::printf(" %d", i);
			std::printf("\n");
		}
	}
}

void do_decide() {
	fr::Attempt t;
	t.flags = (int32_t)rd(); t.status = (int32_t)rd();
	for (int k = 0; k < 4; ++k) t.stamp[k] = rd();
	for (int k = 0; k < 4; ++k) t.limits[k] = rd();
	t.attempts_left = (int32_t)rd();
	t.budget_flux = rd_f64();
	t.H = (int32_t)rd(); t.W = (int32_t)rd();
	std::vector<uint8_t> mask((size_t)t.H * t.W);
	std::vector<double> sum((size_t)t.H * t.W);
	for (auto& v : mask) v = (uint8_t)rd();
	for (auto& v : sum) v = rd_f64();
	t.mask = mask.data(); t.sumimage = sum.data();
	const fr::Decision d = fr::decide_target(t);
	std::printf("%d %d %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %016" PRIx64 " %d", (int)d.outcome, d.status, (int)d.moved,
		d.stamp[0], d.stamp[1], d.stamp[2], d.stamp[3], d.kind, bits(d.edge_flux), d.n_codes);
	for (int k = 0; k < d.n_codes; ++k) std::printf(" %d", d.codes[k]);
	std::printf("\n");
}

} // namespace

int main() {
	fr::CatalogIndex index;
	std::string cmd;
	while (std::cin >> cmd) {
		if (cmd == "size_class") {
			const int64_t k = rd();
			for (int64_t i = 0; i < k; ++i) std::printf("%zu ", fr::size_class((size_t)rd()));
			std::printf("\n");
		} else if (cmd == "pairwise") {
			std::vector<double> a((size_t)rd());
			for (auto& v : a) v = rd_f64();
			std::printf("%016" PRIx64 "\n", bits(fr::np_pairwise_sum(a.data(), (int64_t)a.size())));
		} else if (cmd == "catalog") {
			const int64_t n = rd();
			std::vector<int64_t> sid((size_t)n); std::vector<float> tmag((size_t)n); std::vector<double> row((size_t)n), col((size_t)n);
			for (int64_t i = 0; i < n; ++i) { sid[(size_t)i] = rd(); tmag[(size_t)i] = rd_f32(); row[(size_t)i] = rd_f64(); col[(size_t)i] = rd_f64(); }
			index = fr::CatalogIndex();
			index.build(n, sid.data(), tmag.data(), row.data(), col.data());
		} else if (cmd == "select") {
			do_select(index);
		} else if (cmd == "block") {
			const int64_t m = rd(), T = rd(), H = rd(), W = rd(), cap = rd();
			const fr::BlockLayout b(m, T, H, W, cap);
			for (int f = 0; f < fr::BlockLayout::N_FIELDS; ++f) std::printf("%" PRIu64 " ", b.off[f]);
			std::printf("%" PRIu64 "\n", b.nbytes);
		} else if (cmd == "meta") {
			const int64_t T = rd(), m = rd(), nc = rd();
			const fr::MetaLayout l(T, m, nc);
			for (int f = 0; f < fr::MetaLayout::N_FIELDS; ++f) std::printf("%zu ", l.off[f]);
			std::printf("%zu\n", l.nbytes);
		} else if (cmd == "plan") {
			do_plan();
		} else if (cmd == "decide") {
			do_decide();
		} else { std::printf("FAILED: unknown command '%s'\n", cmd.c_str()); return 2; }
	}
	return 0;
}
