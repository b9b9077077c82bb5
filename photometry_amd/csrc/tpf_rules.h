// tpf_rules.h -- what the target-pixel-file unpacker decides (tpfin.hip), each rule stated once over plain values: the argument
// checks of tp_tpf_unpack (the kept-row list among them), the tile geometry -- constants, grid size, which element of a tile a
// thread loads and which it stores --, the LDS index, where a value lies in the table and in the cube, and the pad range.  No
// device code, no HIP runtime: the kernel calls these from its parallel plumbing, tests/hostsim/tpf_rules_host.cpp composes them
// serially into a complete unpack under AddressSanitizer and UBSan, and tests/test_tpf_host.py holds that to numpy.
#pragma once
#include <cstdint>
#include "fits_rules.h"

namespace tp_tpf {

constexpr int kThreads = 256;     // a workgroup: four wavefronts
constexpr int kTileT = 64;        // cadences of a tile: the lanes of a wavefront when it stores
constexpr int kTileP = 64;        // pixels of a tile: the lanes of a wavefront when it loads
constexpr int kLdsPitch = 65;     // dwords between two cadences of the LDS tile: odd, see tpfin.hip
constexpr int kLdsWords = kTileT * kLdsPitch;
constexpr int kSteps = kTileT * kTileP / kThreads;   // elements a thread loads, and stores: 16
constexpr int kMaxCols = 4;       // image columns of one launch (blockIdx.z)
constexpr int64_t kMaxPix = 1 << 22;                 // pixels of a stamp: blockIdx.y stays below 65536
constexpr int64_t kMaxPitch = (int64_t)1 << 36;      // cadences of a pixel's series with their padding: blockIdx.x stays below 2^30
constexpr int64_t kMaxRows = ((int64_t)1 << 31) - 1; // row numbers travel as int32

using tp_fits::bswap32;

// the kept rows: T row numbers of the table, strictly increasing, each in [0, n_rows)
inline const char* rows_check(const int32_t* rows, int64_t T, int64_t n_rows)
{
	for (int64_t k = 0; k < T; k++) {
		if (!(rows[k] >= 0 && rows[k] < n_rows)) return "tp_tpf_unpack: a kept row lies outside the table";
		if (k > 0 && !(rows[k] > rows[k - 1])) return "tp_tpf_unpack: the kept rows must increase strictly";
	}
	return nullptr;
}

// the message of the first rule a call breaks, or null.  Addresses travel as integers; `rows` is host memory (or null: all rows).
inline const char* unpack_check(uint64_t table_addr, int64_t row_bytes, int64_t n_rows, const int32_t* rows, int64_t T, int32_t n_cols,
	const int64_t* col_offsets, int64_t n_pix, const uint64_t* out_addrs, int64_t t_pitch)
{
	if (table_addr == 0 || col_offsets == nullptr || out_addrs == nullptr) return "tp_tpf_unpack: null pointer";
	if (!(n_cols >= 1 && n_cols <= kMaxCols)) return "tp_tpf_unpack: n_cols must lie in [1, 4]";
	for (int c = 0; c < n_cols; c++)
		if (out_addrs[c] == 0) return "tp_tpf_unpack: null pointer";
	if (table_addr % 4 != 0) return "tp_tpf_unpack: d_table must be 4-byte aligned";
	for (int c = 0; c < n_cols; c++)
		if (out_addrs[c] % 4 != 0) return "tp_tpf_unpack: the output cubes must be 4-byte aligned";
	if (!(row_bytes >= 4 && row_bytes % 4 == 0)) return "tp_tpf_unpack: row_bytes must be a positive multiple of 4";
	if (!(n_pix >= 1 && n_pix <= kMaxPix)) return "tp_tpf_unpack: n_pix must lie in [1, 2^22]";
	for (int c = 0; c < n_cols; c++) {
		if (!(col_offsets[c] >= 0 && col_offsets[c] % 4 == 0)) return "tp_tpf_unpack: a column offset must be a non-negative multiple of 4";
		if (!(col_offsets[c] <= row_bytes - 4 * n_pix)) return "tp_tpf_unpack: a column leaves the row";
	}
	if (!(n_rows >= 1 && n_rows <= kMaxRows)) return "tp_tpf_unpack: n_rows must lie in [1, 2^31)";
	if ((uint64_t)row_bytes >= tp_fits::kMaxSumBytes || (uint64_t)n_rows * (uint64_t)row_bytes >= tp_fits::kMaxSumBytes)
		return "tp_tpf_unpack: a data unit holds fewer than 2^34 bytes";
	if (!(T >= 1 && T <= n_rows)) return "tp_tpf_unpack: T must lie in [1, n_rows]";
	if (rows == nullptr && T != n_rows) return "tp_tpf_unpack: without a list of kept rows T must equal n_rows";
	if (!(t_pitch >= T && t_pitch % 32 == 0 && t_pitch <= kMaxPitch)) return "tp_tpf_unpack: t_pitch must be a multiple of 32, at least T";
	if (rows != nullptr) return rows_check(rows, T, n_rows);
	return nullptr;
}

// tiles along the cadences (the pad cadences [T, t_pitch) belong to tiles too) and along the pixels
TP_RULE inline int64_t grid_t(int64_t t_pitch) { return (t_pitch + kTileT - 1) / kTileT; }
TP_RULE inline int64_t grid_p(int64_t n_pix) { return (n_pix + kTileP - 1) / kTileP; }

// The element (cadence tt, pixel pp) of its tile that thread `thread` moves in step `step` of kSteps.  Loading, the 64 lanes of a
// wavefront are 64 consecutive pixels of one cadence (256 contiguous bytes of a table row) and the wavefronts take every fourth
// cadence; storing, the lanes are 64 consecutive cadences of one pixel (256 contiguous bytes of the cube) and the wavefronts take
// every fourth pixel.  Over threads and steps each map covers the tile exactly once.
struct TileElem {
	int tt, pp;
};
TP_RULE inline TileElem load_elem(int thread, int step) { return TileElem{(thread >> 6) + (kThreads >> 6) * step, thread & 63}; }
TP_RULE inline TileElem store_elem(int thread, int step) { return TileElem{thread & 63, (thread >> 6) + (kThreads >> 6) * step}; }

// where element (tt, pp) of a tile lies in LDS, in dwords
TP_RULE inline int lds_index(int tt, int pp) { return tt * kLdsPitch + pp; }

// byte of the table at which pixel `pixel` of the column at `col_offset` of table row `row` begins
TP_RULE inline int64_t src_byte(int64_t row, int64_t row_bytes, int64_t col_offset, int64_t pixel) { return row * row_bytes + col_offset + 4 * pixel; }
// value of the cube [n_pix][t_pitch] that holds cadence t of pixel `pixel`
TP_RULE inline int64_t dst_index(int64_t pixel, int64_t t, int64_t t_pitch) { return pixel * t_pitch + t; }

// what is stored at cadence t of a pixel's series: a value of the table, the 0.0 of the pad cadences [T, t_pitch), or nothing
enum StoreKind { kStoreNone = 0, kStoreValue = 1, kStorePad = 2 };
TP_RULE inline int store_kind(int64_t t, int64_t T, int64_t t_pitch) { return t < T ? kStoreValue : t < t_pitch ? kStorePad : kStoreNone; }

} // namespace tp_tpf
