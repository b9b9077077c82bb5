// Host driver of the LinPSF plan's device-free rules (photometry_amd/csrc/linpsf_plan_rules.h), built with
// -fsanitize=address,undefined by tests/test_linpsf_plan_host.py.  It composes the rules SERIALLY into the plan of a target -- where
// tp_linpsf_plan_kernel reduces over lanes and scans windows of tiles, it grows a range tile by tile and closes a segment when the
// span test fails -- and prints what the plan holds.  Input on stdin (tokens separated by white space, doubles as the hexadecimal
// bit pattern):
//   constants                                            -> "constants" and the header's constants
//   target H W cutoff path S T, then S x T x (valid ax0 by0 row col)
//     -> path P                                          (3: more than kMaxStars stars, the many-star kernel's: nothing else follows)
//        star s nc axmin bymin nby jmin jmax imin imax item_off
//        nseg N, then per segment: seg tile0 tile1 kdoubles koff, and per star: segstar axmin bymin na nb ksub
//        npix N                                          (-1: the union list was not made)
//        keys .. / ulist .. / usig ..                    (sorted keys and the list, N <= kMfmaPixels entries each)
//        tiles s tiles edge_tiles                        (per star of the matrix-core path)
//        items N                                         (polynomial items of the target, -1 unless it takes the polynomial path)
//        ckeys .. / corder ..                            (polynomial path, T <= 8192: the sort key of every cadence; the cadences in sorted order)
//        end
#include "linpsf_plan_rules.h"
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace tp_linpsf;

namespace {

[[noreturn]] void fail(const char* what) { std::printf("FAILED: %s\n", what); std::exit(1); }
int64_t rd() { long long v; if (!(std::cin >> v)) fail("input ended"); return (int64_t)v; }
double rd_f64() { std::string s; if (!(std::cin >> s)) fail("input ended"); const uint64_t b = std::strtoull(s.c_str(), nullptr, 16); double v; std::memcpy(&v, &b, 8); return v; }

struct Cadence { bool valid; int ax0, by0; double row, col; };

struct Target {
	int H, W, path, ns, T;
	double cutoff;
	std::vector<Cadence> cad;   // [ns][T]
	const Cadence& at(int s, int k) const { return cad[(size_t)s * T + k]; }
};

// the interval ranges of star s in tile t of cadences, as the walk reads them
void tile_ranges(const Target& g, int s, int t, int (&lo)[2], int (&hi)[2])
{
	lo[0] = lo[1] = kTileNone; hi[0] = hi[1] = kTileNoneHigh;
	for (int k = 16 * t; k < 16 * t + 16 && k < g.T; ++k) {
		const Cadence& c = g.at(s, k);
		if (!c.valid) continue;
		const int v[2] = {tile_record(c.ax0), tile_record(c.by0)};
		for (int e = 0; e < 2; ++e) { lo[e] = v[e] < lo[e] ? v[e] : lo[e]; hi[e] = v[e] > hi[e] ? v[e] : hi[e]; }
	}
}

// the greedy segmentation, one tile at a time; 0 segments: a tile alone goes beyond the span, or more than kMfmaSegs are needed
int walk_tiles(const Target& g, const StarPlan* spl, SegPlan* seg)
{
	const int ntile = (g.T + 15) >> 4, ns = g.ns;
	int clo[kMfmaStars][2], chi[kMfmaStars][2];
	ranges_clear(clo, chi);
	int nseg = 0, seg_start = 0;
	for (int t = 0; t < ntile; ++t) {
		for (int attempt = 0; ; ++attempt) {
			int nlo[kMfmaStars][2], nhi[kMfmaStars][2];
			bool fits = true;
			for (int s = 0; s < kMfmaStars; ++s) {
				int lo[2] = {kTileNone, kTileNone}, hi[2] = {kTileNoneHigh, kTileNoneHigh};
				if (s < ns) tile_ranges(g, s, t, lo, hi);
				for (int e = 0; e < 2; ++e) {
					nlo[s][e] = clo[s][e] < lo[e] ? clo[s][e] : lo[e]; nhi[s][e] = chi[s][e] > hi[e] ? chi[s][e] : hi[e];
					if (!span_fits(nlo[s][e], nhi[s][e])) fits = false;
				}
			}
			if (fits) { std::memcpy(clo, nlo, sizeof(clo)); std::memcpy(chi, nhi, sizeof(chi)); break; }
			if (attempt == 1 || t == seg_start) return 0;   // one tile of cadences alone goes beyond the span
			if (nseg >= kMfmaSegs) return 0;
			emit_segment(seg[nseg++], 0, seg_start, t, clo, chi, ns, spl);
			seg_start = t;
			ranges_clear(clo, chi);
		}
	}
	if (nseg >= kMfmaSegs) return 0;
	emit_segment(seg[nseg++], 0, seg_start, ntile, clo, chi, ns, spl);
	return nseg;
}

bool same_segment(const SegPlan& a, const SegPlan& b)
{
	bool same = a.tile0 == b.tile0 && a.tile1 == b.tile1;
	for (int s = 0; s < kMfmaStars; ++s) same = same && a.axmin[s] == b.axmin[s] && a.bymin[s] == b.bymin[s] && a.na[s] == b.na[s] && a.nb[s] == b.nb[s];
	return same;
}

void do_target()
{
	Target g;
	g.H = (int)rd(); g.W = (int)rd(); g.cutoff = rd_f64(); g.path = (int)rd(); g.ns = (int)rd(); g.T = (int)rd();
	g.cad.resize((size_t)g.ns * g.T);
	for (auto& c : g.cad) { c.valid = rd() != 0; c.ax0 = (int)rd(); c.by0 = (int)rd(); c.row = rd_f64(); c.col = rd_f64(); }
	const int ns = g.ns;
	if (ns > kMaxStars) { std::printf("path 3\nend\n"); return; }

	// the boxes and the rectangles the positions sweep
	StarBox sbox[kMaxStars];
	StarPlan spl[kMaxStars];
	double srange[kMaxStars][4];
	for (int s = 0; s < ns; ++s) {
		box_clear(sbox[s]);
		int lo[4] = {kBoxNone, kBoxNone, kBoxNone, kBoxNone}, hi[4] = {-kBoxNone, -kBoxNone, -kBoxNone, -kBoxNone};
		double* pr = srange[s];
		pr[0] = 1e300; pr[1] = -1e300; pr[2] = 1e300; pr[3] = -1e300;
		for (int k = 0; k < g.T; ++k) {
			const Cadence& c = g.at(s, k);
			if (!c.valid) continue;
			int v0[4], v1[4];
			cadence_box(c.ax0, c.by0, c.row, c.col, g.cutoff, v0, v1);
			for (int e = 0; e < 4; ++e) { lo[e] = v0[e] < lo[e] ? v0[e] : lo[e]; hi[e] = v1[e] > hi[e] ? v1[e] : hi[e]; }
			pr[0] = fmin(pr[0], c.row); pr[1] = fmax(pr[1], c.row); pr[2] = fmin(pr[2], c.col); pr[3] = fmax(pr[3], c.col);
		}
		if (hi[0] >= lo[0]) sbox[s] = StarBox{lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3]};
		star_plan_of(sbox[s], g.H, g.W, spl[s]);
	}
	const int fallback = fallback_path(spl, ns);

	// the segments
	SegPlan seg[kMfmaSegs];
	int nseg = 0;
	if (segments_possible(want_segments(g.path, ns), g.H, g.W, g.T)) {
		nseg = walk_tiles(g, spl, seg);
		int lo[kMfmaStars][2], hi[kMfmaStars][2];
		if (whole_series_ranges(sbox, ns, lo, hi)) {
			// the shortcut the kernel takes must be what the walk finds
			SegPlan whole;
			emit_segment(whole, 0, 0, (g.T + 15) >> 4, lo, hi, ns, spl);
			if (nseg != 1 || !same_segment(whole, seg[0])) fail("the whole-series segment is not the walk's");
		}
	}
	int path = (nseg > 0) ? kPathMfma : fallback;

	// the union list
	int nk = -1;
	std::vector<unsigned> keys;
	unsigned tiles[kMfmaStars] = {0u, 0u, 0u, 0u}, etiles[kMfmaStars] = {0u, 0u, 0u, 0u};
	std::vector<uint16_t> ulist(kMfmaPixels, (uint16_t)0xffffu);
	std::vector<uint8_t> usig(kMfmaPixels, (uint8_t)0);
	if (path == kPathMfma) {
		const double reach = pixel_reach2(g.cutoff), always = pixel_always2(g.cutoff);
		nk = 0;
		for (int p = 0; p < g.H * g.W; ++p) {
			const int i = p / g.W, j = p - i * g.W;
			unsigned sig = 0u, edge = 0u;
			for (int s = 0; s < ns; ++s) {
				if (spl[s].nc <= 0) continue;
				const unsigned m = pixel_membership(i, j, srange[s], reach, always);
				sig |= (m & 1u) << s; edge |= (m >> 1) << s;
			}
			if (sig) { if (nk < kMfmaPixels) keys.push_back(pixel_key(sig, edge, p)); ++nk; }
		}
		if (nk > kMfmaPixels) path = fallback;
		else for (unsigned key : keys) {
			int r = 0;
			for (unsigned other : keys) r += (other < key) ? 1 : 0;
			ulist[(size_t)r] = key_pixel(key); usig[(size_t)r] = key_usig(key);
			for (int s = 0; s < ns; ++s) {
				if (key_sig(key) & (1u << s)) tiles[s] |= 1u << (r >> 4);
				if (key_edge(key) & (1u << s)) etiles[s] |= 1u << (r >> 4);
			}
		}
	}

	// the coefficient images, or the polynomial items
	MPlan mp;
	make_mplan(mp, nk < 0 ? 0 : nk, nseg, ns, tiles, etiles);
	const bool listed = nk >= 0 && nk <= kMfmaPixels;
	if (path == kPathMfma) {
		long long total;
		if (!size_segments(seg, nseg, ns, mp, total)) path = fallback;
	}
	long long items = -1;
	if (path == kPathPoly) items = poly_item_offsets(spl, ns);

	std::printf("path %d\n", path);
	for (int s = 0; s < ns; ++s) {
		const StarPlan& q = spl[s];
		std::printf("star %d %d %d %d %d %d %d %d %d %lld\n", s, q.nc, q.axmin, q.bymin, q.nby, q.jmin, q.jmax, q.imin, q.imax, q.item_off);
	}
	std::printf("nseg %d\n", nseg);
	for (int i = 0; i < nseg; ++i) {
		std::printf("seg %d %d %d %lld\n", (int)seg[i].tile0, (int)seg[i].tile1, listed ? (int)seg[i].kdoubles : -1, listed ? (long long)seg[i].koff : -1ll);
		for (int s = 0; s < ns; ++s) std::printf("segstar %d %d %d %d %d\n", (int)seg[i].axmin[s], (int)seg[i].bymin[s], (int)seg[i].na[s], (int)seg[i].nb[s], listed ? (int)seg[i].ksub[s] : -1);
	}
	std::printf("npix %d\n", nk);
	if (listed) {
		std::vector<unsigned> sorted(keys.size());
		for (unsigned key : keys) { size_t r = 0; for (unsigned other : keys) r += (other < key) ? 1 : 0; sorted[r] = key; }
		std::printf("keys"); for (unsigned k : sorted) std::printf(" %u", k); std::printf("\n");
		std::printf("ulist"); for (int r = 0; r < nk; ++r) std::printf(" %u", (unsigned)ulist[(size_t)r]); std::printf("\n");
		std::printf("usig"); for (int r = 0; r < nk; ++r) std::printf(" %u", (unsigned)usig[(size_t)r]); std::printf("\n");
		for (int s = 0; s < ns && s < kMfmaStars; ++s) std::printf("tiles %d %u %u\n", s, (unsigned)mp.tiles[s], (unsigned)mp.edge_tiles[s]);
	}
	std::printf("items %lld\n", items);
	if (path == kPathPoly && g.T <= 8192) {
		// the order of the cadences: the key of every cadence, and the cadences read back from the sorted keys
		std::vector<unsigned long long> ckeys((size_t)g.T);
		for (int k = 0; k < g.T; ++k) {
			unsigned long long key = 0;
			for (int s = 0; s < ns; ++s) key = cadence_key_star(key, spl[s], g.at(s, k).valid, g.at(s, k).ax0, g.at(s, k).by0);
			ckeys[(size_t)k] = cadence_key_close(key, k);
		}
		std::printf("ckeys"); for (unsigned long long k : ckeys) std::printf(" %llu", k); std::printf("\n");
		std::sort(ckeys.begin(), ckeys.end());
		std::printf("corder"); for (unsigned long long k : ckeys) std::printf(" %d", key_cadence(k)); std::printf("\n");
	}
	std::printf("end\n");
}

} // namespace

int main()
{
	std::string cmd;
	while (std::cin >> cmd) {
		if (cmd == "constants") {
			std::printf("constants %d %d %d %d %d %d %d %d %d\n", kMaxStars, kMfmaStars, kMfmaPixels, kMfmaSpan, kMfmaSegs, kMfmaCadTiles, kMfmaLdsSmall, kMfmaLdsLarge, kMaxOrigins);
			std::printf("steps %d %d %d %d\n", mfma_steps(1, 1), mfma_steps(2, 2), mfma_steps(3, 3), mfma_steps(3, 2));
		}
		else if (cmd == "target") do_target();
		else fail("unknown command");
	}
	return 0;
}
