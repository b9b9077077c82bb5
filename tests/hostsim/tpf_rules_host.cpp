// Host driver of the target-pixel-file unpacker's device-free rules (photometry_amd/csrc/tpf_rules.h), built with
// -fsanitize=address,undefined by tests/test_tpf_host.py.  It reads commands from stdin (tokens separated by white space; addresses
// travel in hexadecimal) and answers every command with lines on stdout:
//   check N, then N x (table_addr row_bytes n_rows T n_cols off0 off1 off2 off3 n_pix out0 out1 out2 out3 t_pitch nr r1 .. r_nr;
//     nr = -1: no list of kept rows; n_cols = -1: null offsets, -2: null outputs (n_cols then counts as 1))
//                                          -> N x "ok" | "refused MSG"
//   maps 1                                 -> "ok" when load_elem, store_elem and lds_index each cover a tile exactly once without
//                                             two elements on one LDS word, else "FAILED: ..."
//   unpack 1, then table_file out_file row_bytes n_rows T n_cols off0 off1 off2 off3 n_pix t_pitch nr r1 .. r_nr
//                                          -> "refused MSG", or the rules composed serially into a complete unpack -- every block of
//                                             the grid, every thread, every step, first the loads into a tile of LDS size, then the
//                                             stores -- of the table in table_file (exactly n_rows * row_bytes bytes) into n_cols
//                                             cubes [n_pix][t_pitch] pre-filled with a sentinel, written to out_file as native uint32;
//                                             "ok writes W min A max B": stores in all, fewest and most per output element
#include "tpf_rules.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using namespace tp_tpf;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
uint64_t rd_hex() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return std::strtoull(s.c_str(), nullptr, 16); }
std::string rd_str() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return s; }

std::vector<int32_t> rd_rows(int64_t nr)
{
	std::vector<int32_t> rows;
	for (int64_t k = 0; k < nr; k++) rows.push_back((int32_t)rd());
	return rows;
}

int maps()
{
	std::vector<int> loaded(kTileT * kTileP, 0), stored(kTileT * kTileP, 0), word(kLdsWords, 0);
	for (int thread = 0; thread < kThreads; thread++)
		for (int step = 0; step < kSteps; step++) {
			const TileElem a = load_elem(thread, step), b = store_elem(thread, step);
			if (a.tt < 0 || a.tt >= kTileT || a.pp < 0 || a.pp >= kTileP || b.tt < 0 || b.tt >= kTileT || b.pp < 0 || b.pp >= kTileP) { std::printf("FAILED: element off the tile\n"); return 1; }
			loaded[a.tt * kTileP + a.pp]++;
			stored[b.tt * kTileP + b.pp]++;
			word[lds_index(a.tt, a.pp)]++;
			// a wavefront loads one cadence, and stores one pixel
			if (a.pp != (thread & 63) || b.tt != (thread & 63)) { std::printf("FAILED: the lanes of a wavefront are not consecutive\n"); return 1; }
			if (a.tt != load_elem(thread & ~63, step).tt || b.pp != store_elem(thread & ~63, step).pp) { std::printf("FAILED: a wavefront is split\n"); return 1; }
		}
	for (int i = 0; i < kTileT * kTileP; i++)
		if (loaded[i] != 1 || stored[i] != 1) { std::printf("FAILED: element %d loaded %d times, stored %d times\n", i, loaded[i], stored[i]); return 1; }
	for (int i = 0; i < kLdsWords; i++)
		if (word[i] > 1) { std::printf("FAILED: LDS word %d holds %d elements\n", i, word[i]); return 1; }
	if (kLdsPitch % 2 != 1 || kLdsPitch < kTileP) { std::printf("FAILED: LDS pitch\n"); return 1; }
	std::printf("ok\n");
	return 0;
}

int unpack()
{
	const std::string table_file = rd_str(), out_file = rd_str();
	const int64_t row_bytes = rd(), n_rows = rd(), T = rd();
	const int32_t n_cols = (int32_t)rd();
	int64_t offs[kMaxCols];
	for (auto& o : offs) o = rd();
	const int64_t n_pix = rd(), t_pitch = rd(), nr = rd();
	const std::vector<int32_t> rows = rd_rows(nr < 0 ? 0 : nr);
	const int32_t* h_rows = nr < 0 ? nullptr : rows.data();

	std::ifstream in(table_file, std::ios::binary);
	std::vector<unsigned char> table((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	if (row_bytes > 0 && n_rows > 0 && (int64_t)table.size() != row_bytes * n_rows) { std::printf("FAILED: %zu bytes in the table file\n", table.size()); return 1; }
	constexpr uint32_t kSentinel = 0xDEADBEEFu;
	const bool sized = n_cols >= 1 && n_cols <= kMaxCols && n_pix >= 1 && n_pix <= kMaxPix && t_pitch >= 1 && t_pitch <= (1 << 24);
	std::vector<std::vector<uint32_t>> out(kMaxCols);
	std::vector<std::vector<int32_t>> count(kMaxCols);
	uint64_t out_addrs[kMaxCols] = {0, 0, 0, 0};
	for (int c = 0; sized && c < n_cols; c++) {
		out[c].assign((size_t)(n_pix * t_pitch), kSentinel);
		count[c].assign((size_t)(n_pix * t_pitch), 0);
		out_addrs[c] = reinterpret_cast<uintptr_t>(out[c].data());
	}
	const char* msg = unpack_check(reinterpret_cast<uintptr_t>(table.data()), row_bytes, n_rows, h_rows, T, n_cols, offs, n_pix, out_addrs, t_pitch);
	if (msg) { std::printf("refused %s\n", msg); return 0; }

	for (int64_t bz = 0; bz < n_cols; bz++)
		for (int64_t by = 0; by < grid_p(n_pix); by++)
			for (int64_t bx = 0; bx < grid_t(t_pitch); bx++) {
				std::vector<uint32_t> tile(kLdsWords, 0xA5A5A5A5u);         // a block's LDS: exactly its size, stale before the loads
				std::vector<char> fresh(kLdsWords, 0);
				const int64_t t0 = bx * kTileT, p0 = by * kTileP;
				if (t0 < T)
					for (int thread = 0; thread < kThreads; thread++)
						for (int step = 0; step < kSteps; step++) {
							const TileElem e = load_elem(thread, step);
							const int64_t t = t0 + e.tt, pixel = p0 + e.pp;
							if (t < T && pixel < n_pix) {
								const int64_t row = h_rows ? (int64_t)h_rows[t] : t;
								uint32_t v;
								std::memcpy(&v, &table.at((size_t)src_byte(row, row_bytes, offs[bz], pixel)), 4);
								(void)table.at((size_t)src_byte(row, row_bytes, offs[bz], pixel) + 3);
								tile.at(lds_index(e.tt, e.pp)) = bswap32(v);
								fresh.at(lds_index(e.tt, e.pp)) = 1;
							}
						}
				for (int thread = 0; thread < kThreads; thread++)
					for (int step = 0; step < kSteps; step++) {
						const TileElem e = store_elem(thread, step);
						const int64_t t = t0 + e.tt, pixel = p0 + e.pp;
						if (pixel >= n_pix) continue;
						const int kind = store_kind(t, T, t_pitch);
						if (kind == kStoreNone) continue;
						if (kind == kStoreValue && !fresh.at(lds_index(e.tt, e.pp))) { std::printf("FAILED: a store reads an LDS word no load wrote\n"); return 1; }
						out[bz].at((size_t)dst_index(pixel, t, t_pitch)) = kind == kStoreValue ? tile.at(lds_index(e.tt, e.pp)) : 0u;
						count[bz].at((size_t)dst_index(pixel, t, t_pitch))++;
					}
			}
	int64_t writes = 0;
	int32_t lo = INT32_MAX, hi = 0;
	std::ofstream of(out_file, std::ios::binary);
	for (int c = 0; c < n_cols; c++) {
		for (int32_t n : count[c]) { writes += n; lo = n < lo ? n : lo; hi = n > hi ? n : hi; }
		of.write(reinterpret_cast<const char*>(out[c].data()), (std::streamsize)(out[c].size() * 4));
	}
	std::printf("ok writes %" PRId64 " min %d max %d\n", writes, lo, hi);
	return 0;
}

} // namespace

int main()
{
	std::string cmd;
	while (std::cin >> cmd) {
		const int64_t n = rd();
		if (cmd == "check") {
			for (int64_t i = 0; i < n; i++) {
				const uint64_t table = rd_hex();
				const int64_t row_bytes = rd(), n_rows = rd(), T = rd();
				const int32_t n_cols = (int32_t)rd();
				int64_t offs[kMaxCols];
				for (auto& o : offs) o = rd();
				const int64_t n_pix = rd();
				uint64_t outs[kMaxCols];
				for (auto& o : outs) o = rd_hex();
				const int64_t t_pitch = rd(), nr = rd();
				const std::vector<int32_t> rows = rd_rows(nr < 0 ? 0 : nr);
				const char* msg = unpack_check(table, row_bytes, n_rows, nr < 0 ? nullptr : rows.data(), T, n_cols < 0 ? 1 : n_cols, n_cols == -1 ? nullptr : offs, n_pix,
					n_cols == -2 ? nullptr : outs, t_pitch);
				if (msg) std::printf("refused %s\n", msg);
				else std::printf("ok\n");
			}
		} else if (cmd == "maps") {
			if (maps()) return 1;
		} else if (cmd == "unpack") {
			if (unpack()) return 1;
		} else {
			std::printf("FAILED: unknown command %s\n", cmd.c_str());
			return 1;
		}
	}
	return 0;
}
