// Host driver of the per-target star positions' device-free rules (photometry_amd/csrc/starpos_rules.h), built with
// -fsanitize=address,undefined by tests/test_tpf_linpsf_host.py.  It reads commands from stdin (tokens separated by white space):
//   grid 1                                 -> "ok" when the grid owns every (star, cadence) pair exactly once, else "FAILED: ..."
//   positions 1, then n_stars n_cad n_targets shift_pitch has_lookup lookup_pitch pos_pitch null (0 none, 1 base, 2 star_target,
//     3 shift, 4 output), then n_stars float32 bit patterns (hex) of the bases, n_stars targets, n_targets * shift_pitch float64 bit
//     patterns (hex) of the shifts and, with has_lookup, n_targets * lookup_pitch rows
//                                          -> "refused MSG", or "ok writes W max M" (stores in all, most per value) and then one line
//                                             per star: pos_pitch float64 bit patterns (hex) of the rules composed serially -- every
//                                             block of the grid, every thread, every star a block walks -- into [n_stars][pos_pitch]
//                                             pre-filled with a sentinel.  Every array holds exactly the values the call may touch.
#include "starpos_rules.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace tp_starpos;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
uint64_t rd_hex() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return std::strtoull(s.c_str(), nullptr, 16); }

constexpr uint64_t kSentinel = 0x7ff8dead0000beefull;

int grid()
{
	for (int64_t T : {1, 255, 256, 257, 300, 1000})
		for (int64_t N : {1, 2, 11}) {
			std::vector<int> seen((size_t)(T * N), 0);
			for (int64_t by = 0; by < blocks_y(N); by++)
				for (int64_t bx = 0; bx < blocks_x(T); bx++)
					for (int thread = 0; thread < kThreads; thread++) {
						const int64_t k = cadence_of(bx, thread);
						if (k >= T) continue;
						for (int64_t s = by; s < N; s += blocks_y(N)) seen.at((size_t)pos_index(s, k, T))++;
					}
			for (int n : seen)
				if (n != 1) { std::printf("FAILED: a (star, cadence) pair owned %d times\n", n); return 1; }
		}
	// more stars than the grid is high: a block walks several
	const int64_t N = kMaxGridY * 2 + 5;
	if (blocks_y(N) != kMaxGridY) { std::printf("FAILED: blocks_y\n"); return 1; }
	std::vector<int> seen((size_t)N, 0);
	for (int64_t by = 0; by < blocks_y(N); by++)
		for (int64_t s = by; s < N; s += blocks_y(N)) seen.at((size_t)s)++;
	for (int n : seen)
		if (n != 1) { std::printf("FAILED: a star walked %d times\n", n); return 1; }
	std::printf("ok\n");
	return 0;
}

int positions()
{
	const int64_t n_stars = rd(), n_cad = rd(), n_targets = rd(), shift_pitch = rd(), has_lookup = rd(), lookup_pitch = rd(), pos_pitch = rd(), null = rd();
	const auto count = [](int64_t a, int64_t b) { return (a > 0 && b > 0 && a <= (1 << 20) && b <= (1 << 20)) ? (size_t)(a * b) : (size_t)0; };
	std::vector<float> base(count(n_stars, 1));
	std::vector<int32_t> star_target(count(n_stars, 1));
	std::vector<double> shift(count(n_targets, shift_pitch));
	std::vector<int32_t> lookup(has_lookup ? count(n_targets, lookup_pitch) : 0);
	for (float& v : base) { const uint32_t bits = (uint32_t)rd_hex(); std::memcpy(&v, &bits, 4); }
	for (int32_t& v : star_target) v = (int32_t)rd();
	for (double& v : shift) { const uint64_t bits = rd_hex(); std::memcpy(&v, &bits, 8); }
	for (int32_t& v : lookup) v = (int32_t)rd();
	std::vector<double> pos(count(n_stars, pos_pitch));
	for (double& v : pos) std::memcpy(&v, &kSentinel, 8);
	std::vector<int32_t> stores(pos.size(), 0);

	const char* msg = sizes_check(n_stars, n_cad, n_targets, shift_pitch, has_lookup != 0, lookup_pitch, pos_pitch);
	if (msg) { std::printf("refused %s\n", msg); return 0; }
	if (n_stars > 0 && n_cad > 0) {
		// (an empty vector's data() may be null by itself: the addresses are what the caller would have passed)
		msg = pointers_check(null == 1 ? 0 : 1, null == 2 ? 0 : 1, null == 3 ? 0 : 1, null == 4 ? 0 : 1);
		if (msg) { std::printf("refused %s\n", msg); return 0; }
		const int32_t* lk = has_lookup ? lookup.data() : nullptr;
		for (int64_t by = 0; by < blocks_y(n_stars); by++)
			for (int64_t bx = 0; bx < blocks_x(n_cad); bx++)
				for (int thread = 0; thread < kThreads; thread++) {
					const int64_t k = cadence_of(bx, thread);
					if (k >= n_cad) continue;
					for (int64_t s = by; s < n_stars; s += blocks_y(n_stars)) {
						pos.data()[pos_index(s, k, pos_pitch)] = star_position(base.data(), star_target.data(), shift.data(), shift_pitch, lk, lookup_pitch, n_targets, s, k);
						stores.at((size_t)pos_index(s, k, pos_pitch))++;
					}
				}
	}
	int64_t writes = 0;
	int32_t hi = 0;
	for (int32_t n : stores) { writes += n; hi = n > hi ? n : hi; }
	std::printf("ok writes %" PRId64 " max %d\n", writes, hi);
	for (int64_t s = 0; s < (pos.empty() ? 0 : n_stars); s++) {
		for (int64_t k = 0; k < pos_pitch; k++) {
			uint64_t bits;
			std::memcpy(&bits, &pos[(size_t)pos_index(s, k, pos_pitch)], 8);
			std::printf("%s%016" PRIx64, k ? " " : "", bits);
		}
		std::printf("\n");
	}
	return 0;
}

} // namespace

int main()
{
	std::string cmd;
	while (std::cin >> cmd) {
		(void)rd();
		if (cmd == "grid") {
			if (grid()) return 1;
		} else if (cmd == "positions") {
			if (positions()) return 1;
		} else {
			std::printf("FAILED: unknown command %s\n", cmd.c_str());
			return 1;
		}
	}
	return 0;
}
