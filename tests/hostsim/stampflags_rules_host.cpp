// Host driver of the per-stamp flag series' device-free rules (photometry_amd/csrc/stampflags_rules.h), built with
// -fsanitize=address,undefined by tests/test_stampflags_host.py.  It reads commands from stdin (tokens separated by white space) and
// answers every command with one line on stdout:
//   maps 1                                 -> "ok" when the lane map covers stamps of many shapes exactly once and the grid covers every
//                                             (target, frame) pair exactly once, else "FAILED: ..."
//   series 1, then flags_file out_file n_frames frame_rows frame_cols frame_stride row0 col0 n_targets flag_mask out_value out_pitch
//     null (0 none, 1 flags, 2 stamps, 3 output), then n_targets x (r1 r2 c1 c2)
//                                          -> "refused MSG", or the rules composed serially into a complete series -- every block of
//                                             the grid, every wavefront, every frame of its tile, every step, every lane -- over the
//                                             stack in flags_file (exactly the bytes the call may read: (n_frames - 1) * frame_stride
//                                             + frame_rows * frame_cols) into [n_targets][out_pitch] int32 pre-filled with a sentinel,
//                                             written to out_file; "ok writes W max M": stores in all, most per output element
#include "stampflags_rules.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using namespace tp_sflags;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
std::string rd_str() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return s; }

int maps()
{
	for (int32_t h = 1; h <= 11; h++)
		for (int32_t w = 1; w <= 37; w++) {
			const RelStamp s{3, 3 + h, 5, 5 + w};
			std::vector<int> seen((size_t)(h * w), 0);
			for (int32_t rs = 0; rs < row_steps(s); rs++)
				for (int32_t cs = 0; cs < col_steps(s); cs++)
					for (int lane = 0; lane < kWave; lane++) {
						const int32_t row = lane_row(s, lane, rs), col = lane_col(s, lane, cs);
						if (row < s.r1 || col < s.c1) { std::printf("FAILED: a lane before the stamp\n"); return 1; }
						if (in_stamp(s, row, col)) seen.at((size_t)((row - s.r1) * w + col - s.c1))++;
					}
			for (int n : seen)
				if (n != 1) { std::printf("FAILED: a pixel of a %d x %d stamp read %d times\n", h, w, n); return 1; }
		}
	const RelStamp none{0, 0, 0, 0};
	if (row_steps(none) != 0 || col_steps(none) != 0) { std::printf("FAILED: the empty stamp has steps\n"); return 1; }
	for (int64_t T : {1, 15, 16, 17, 65})
		for (int64_t N : {1, 3, 4, 5, 9}) {
			std::vector<int> seen((size_t)(T * N), 0);
			const int64_t n_groups = groups_n(N);
			for (int64_t block = 0; block < grid_blocks(T, N); block++)
				for (int wave = 0; wave < kWaves; wave++) {
					const int64_t target = block_target(block, n_groups, wave), t0 = block_tile(block, n_groups) * kTileT;
					if (target >= N) continue;
					for (int k = 0; k < kTileT && t0 + k < T; k++) seen.at((size_t)(target * T + t0 + k))++;
				}
			for (int n : seen)
				if (n != 1) { std::printf("FAILED: a (target, frame) pair owned %d times\n", n); return 1; }
		}
	if (kLaneRows * kLaneCols != kWave || kTileT > kWave) { std::printf("FAILED: constants\n"); return 1; }
	std::printf("ok\n");
	return 0;
}

int series()
{
	const std::string flags_file = rd_str(), out_file = rd_str();
	const int64_t n_frames = rd(), frame_rows = rd(), frame_cols = rd(), frame_stride = rd(), row0 = rd(), col0 = rd(), n_targets = rd();
	const uint32_t flag_mask = (uint32_t)rd();
	const int32_t out_value = (int32_t)rd();
	const int64_t out_pitch = rd(), null = rd();
	std::vector<int64_t> stamps;
	for (int64_t i = 0; i < 4 * (n_targets > 0 ? n_targets : 0); i++) stamps.push_back(rd());
	if (stamps.empty()) stamps.assign(4, 0);

	std::ifstream in(flags_file, std::ios::binary);
	std::vector<uint8_t> flags((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	constexpr int32_t kSentinel = -123456789;
	const bool sized = n_targets >= 1 && n_targets <= (1 << 20) && out_pitch >= 1 && out_pitch <= (1 << 20);
	std::vector<int32_t> out(sized ? (size_t)(n_targets * out_pitch) : 1, kSentinel);
	std::vector<int32_t> count(out.size(), 0);
	const char* msg = series_check(null == 1 ? 0 : reinterpret_cast<uintptr_t>(flags.data()), n_frames, frame_rows, frame_cols, frame_stride, row0, col0, n_targets,
		null == 2 ? nullptr : stamps.data(), flag_mask, null == 3 ? 0 : reinterpret_cast<uintptr_t>(out.data()), out_pitch);
	if (msg) { std::printf("refused %s\n", msg); return 0; }
	if ((int64_t)flags.size() != (n_frames - 1) * frame_stride + frame_rows * frame_cols) { std::printf("FAILED: %zu bytes in the flags file\n", flags.size()); return 1; }

	std::vector<RelStamp> rel;
	for (int64_t i = 0; i < n_targets; i++) rel.push_back(relative(stamps.data() + 4 * i, row0, col0));
	const int64_t n_groups = groups_n(n_targets);
	for (int64_t block = 0; block < grid_blocks(n_frames, n_targets); block++)
		for (int wave = 0; wave < kWaves; wave++) {
			const int64_t target = block_target(block, n_groups, wave);
			if (target >= n_targets) continue;
			const int64_t t0 = block_tile(block, n_groups) * kTileT;
			const RelStamp s = rel.at((size_t)target);
			int32_t mine[kWave] = {};
			for (int k = 0; k < kTileT && t0 + k < n_frames; k++) {
				bool any = false;                                          // the ballot
				for (int lane = 0; lane < kWave; lane++) {
					uint32_t seen = 0;
					for (int32_t rs = 0; rs < row_steps(s); rs++)
						for (int32_t cs = 0; cs < col_steps(s); cs++) {
							const int32_t row = lane_row(s, lane, rs), col = lane_col(s, lane, cs);
							if (in_stamp(s, row, col)) seen |= flags.at((size_t)flag_byte(t0 + k, frame_stride, (int32_t)frame_cols, row, col));
						}
					any = any || flagged((uint8_t)seen, flag_mask);
				}
				mine[k] = out_of(any, out_value);
			}
			for (int lane = 0; lane < kWave; lane++)
				if (lane < kTileT && t0 + lane < n_frames) {
					out.at((size_t)out_index(target, t0 + lane, out_pitch)) = mine[lane];
					count.at((size_t)out_index(target, t0 + lane, out_pitch))++;
				}
		}
	int64_t writes = 0;
	int32_t hi = 0;
	for (int32_t n : count) { writes += n; hi = n > hi ? n : hi; }
	std::ofstream of(out_file, std::ios::binary);
	of.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * 4));
	std::printf("ok writes %" PRId64 " max %d\n", writes, hi);
	return 0;
}

} // namespace

int main()
{
	std::string cmd;
	while (std::cin >> cmd) {
		(void)rd();
		if (cmd == "maps") {
			if (maps()) return 1;
		} else if (cmd == "series") {
			if (series()) return 1;
		} else {
			std::printf("FAILED: unknown command %s\n", cmd.c_str());
			return 1;
		}
	}
	return 0;
}
