// Host driver of the cubes path's device-free rules (photometry_amd/csrc/halo_rules.h: CubeGeom, check_cube, check_cube_seg, cube_lists,
// cube_target_of, cube_offset, check_cube_gather, check_cube_norm), built with -fsanitize=address,undefined by
// tests/test_halo_cubes_host.py.  It reads commands from stdin (tokens separated by white space) and answers on stdout:
//   lists n H W T t_pitch bitmask have_cube, prob_off[n + 1], then n x T x (seg quality)
//        -> "cube MSG", "seg MSG" (MSG "ok" for none); when both are ok: "n_prob ..", "target ..", "lo ..", "hi ..", per target "cadlist i ..",
//           "fitlist i ..", then "serial ..": per problem the cadences found by walking the target's row serially through cube_target_of
//           and the problem's [lo, hi) (the indexing the kernels use), "offset ..": cube_offset of (target, pixel) for the four corners
//   tables n H W T t_pitch, prob_off[n + 1], n_run, then n_run x (index p_off npix ncad)
//        -> "gather MSG max_ncad max_pitch", per problem its 6 fields; "norm MSG", per problem its 5 fields, "run .."
#include "halo_rules.h"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <string>

using namespace tp_halo;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
template <class T> void line(const std::string& name, const std::vector<T>& a) { std::printf("%s", name.c_str()); for (auto v : a) std::printf(" %" PRId64, (int64_t)v); std::printf("\n"); }

CubeGeom rd_geom() {
	CubeGeom g;
	g.n_targets = (int32_t)rd(); g.height = (int32_t)rd(); g.width = (int32_t)rd(); g.n_cad = (int32_t)rd(); g.t_pitch = (int32_t)rd();
	g.n_prob = 0;
	return g;
}
std::vector<int32_t> rd_offsets(int n) {
	std::vector<int32_t> off(std::max(n, 0) + 1);
	for (auto& v : off) v = (int32_t)rd();
	return off;
}

void cmd_lists() {
	CubeGeom g = rd_geom();
	const int32_t bitmask = (int32_t)rd();
	const bool have_cube = rd() != 0;
	const std::vector<int32_t> off = rd_offsets(g.n_targets);
	const int64_t cells = (int64_t)std::max(g.n_targets, 0) * std::max(g.n_cad, 0);
	std::vector<int32_t> seg(cells), quality(cells);
	for (int64_t j = 0; j < cells; j++) { seg[j] = (int32_t)rd(); quality[j] = (int32_t)rd(); }
	static const float cube = 0.0f;
	const char* bad = check_cube(g, have_cube ? &cube : nullptr, off.data());
	std::printf("cube %s\n", bad ? bad : "ok");
	if (bad) return;
	bad = check_cube_seg(g, off.data(), seg.data());
	std::printf("seg %s\n", bad ? bad : "ok");
	if (bad) return;
	const CubeLists s = cube_lists(g, off.data(), seg.data(), quality.data(), bitmask);
	std::printf("n_prob %d\n", g.n_prob);
	line("target", s.target);
	line("lo", s.lo);
	line("hi", s.hi);
	const int T = g.n_cad;
	for (int i = 0; i < g.n_targets; i++) {
		line("cadlist " + std::to_string(i), std::vector<int32_t>(s.cadlist.begin() + (int64_t)i * T, s.cadlist.begin() + (int64_t)(i + 1) * T));
		line("fitlist " + std::to_string(i), std::vector<uint8_t>(s.fitlist.begin() + (int64_t)i * T, s.fitlist.begin() + (int64_t)(i + 1) * T));
	}
	// what a kernel's block does for problem q: its target from the offsets, its entries of that target's row
	for (int q = 0; q < g.n_prob; q++) {
		const int i = cube_target_of(off.data(), g.n_targets, q);
		if (i != s.target[q] || !(off[i] <= q && q < off[i + 1])) { std::printf("FAILED: target of problem %d\n", q); std::exit(1); }
		std::vector<int32_t> cad;
		for (int j = s.lo[q]; j < s.hi[q]; j++) {
			const int32_t t = s.cadlist[(int64_t)i * T + j];
			if (!(t >= 0 && t < T) || seg[(int64_t)i * T + t] != q - off[i]) { std::printf("FAILED: cadence %d of problem %d\n", j, q); std::exit(1); }
			cad.push_back(t);
		}
		line("serial " + std::to_string(q), cad);
	}
	const int HW = g.height * g.width;
	line("offset", std::vector<int64_t>{cube_offset(g, 0, 0), cube_offset(g, 0, HW - 1), cube_offset(g, g.n_targets - 1, 0), cube_offset(g, g.n_targets - 1, HW - 1)});
}

void cmd_tables() {
	CubeGeom g = rd_geom();
	const std::vector<int32_t> off = rd_offsets(g.n_targets);
	static const float cube = 0.0f;
	const char* bad = check_cube(g, &cube, off.data());
	if (bad) { std::printf("FAILED: %s\n", bad); std::exit(1); }
	const int n_run = (int)rd();
	std::vector<int32_t> index(n_run), npix(n_run), ncad(n_run);
	std::vector<int64_t> p_off(n_run);
	for (int r = 0; r < n_run; r++) { index[r] = (int32_t)rd(); p_off[r] = rd(); npix[r] = (int32_t)rd(); ncad[r] = (int32_t)rd(); }
	std::vector<GatherProb> gp;
	int32_t max_ncad = 0, max_pitch = 0;
	bad = check_cube_gather(g, n_run, index.data(), p_off.data(), npix.data(), ncad.data(), gp, max_ncad, max_pitch);
	std::printf("gather %s\n", bad ? bad : "ok");
	if (!bad) {
		std::printf("sizes %d %d\n", max_ncad, max_pitch);
		for (const GatherProb& p : gp) std::printf("%" PRId64 " %" PRId64 " %d %d %d %d\n", p.p_off, p.c_off, p.q, p.npix, p.ncad, p.pitch);
	}
	std::vector<NormProb> np;
	std::vector<int32_t> run;
	bad = check_cube_norm(g, n_run, index.data(), npix.data(), ncad.data(), np, run);
	std::printf("norm %s\n", bad ? bad : "ok");
	if (!bad) {
		for (int r = 0; r < n_run; r++) std::printf("%" PRId64 " %" PRId64 " %d %d %d\n", np[r].c_off, np[r].w_off, np[r].q, np[r].npix, np[r].ncad);
		line("run", run);
	}
}

} // namespace

int main() {
	std::string cmd;
	while (std::cin >> cmd) {
		if (cmd == "lists") cmd_lists();
		else if (cmd == "tables") cmd_tables();
		else { std::printf("FAILED: unknown command %s\n", cmd.c_str()); return 1; }
	}
	return 0;
}
