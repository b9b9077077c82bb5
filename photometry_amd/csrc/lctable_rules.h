// lctable_rules.h -- what the light-curve table packer decides (lctable.hip), each rule stated once over plain values: the row layout
// of the LIGHTCURVE table of a FILEVER 1.5 file (lcfile.py: 14 columns `D E J D D D D D J J D D D D`, 96 bytes, big-endian), the value
// conversions, the word sum of a row, the pad, the tile geometry with its LDS index, the segment copy of tp_lc_place, and the
// refusals of both entries.  No device code, no HIP runtime: the kernels call these from their parallel plumbing,
// tests/hostsim/lctable_rules_host.cpp composes them serially into the bytes the kernels write under AddressSanitizer and UBSan, and
// tests/test_lctable_rules_host.py holds that to fitsio.bintable_hdu and fitsio._sum32.
//
// DATASUM without reading a written byte back.  A row is 96 bytes and a data unit begins on a word boundary, so every 32-bit word of
// the data unit lies inside one value: the big-endian words of a 64-bit value v are (v >> 32) and (v & 0xffffffff), in this order, and
// the big-endian word of a 32-bit value is the value.  The sum of the words of a row is therefore the sum of the native halves of its
// eight-byte values and of its native four-byte values (row_sum); the pad behind the last row is zeros and adds nothing; the DATASUM
// of the unit is the 64-bit integer sum of its rows' sums with the carries folded back in (tp_fits::fold32) -- the form
// tp_fits_datasum returns.  Integers only: exact, and the same in every run.
//
// kMaxRows: a row holds 24 words of less than 2^32 each, so the plain 64-bit sum of n rows stays below n * 24 * 2^32 and cannot wrap
// while n <= 2^64 / (24 * 2^32) = 2^32 / 24 = 178 956 970 (rounded down).  tp_lc_table_pack refuses more rows than that.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "fits_rules.h"

namespace tp_lctable {

constexpr int kCols = 14;
constexpr int kRowBytes = 96;                      // NAXIS1
constexpr int kRowWords = kRowBytes / 4;           // 24
constexpr int kRowPieces = kRowBytes / 16;         // 16-byte pieces of a row: 6
constexpr int64_t kBlock = 2880;                   // a FITS block: 30 rows, so the pad is a whole number of rows
constexpr int64_t kBlockRows = kBlock / kRowBytes; // 30
constexpr int kTileRows = 64;                      // rows of a tile: the lanes of a wavefront
constexpr int kWaves = 4;                          // tiles of a workgroup, one per wavefront
constexpr int kThreads = 64 * kWaves;
constexpr int kTileBytes = kTileRows * kRowBytes;  // 6144
constexpr int kTilePieces = kTileRows * kRowPieces; // 384
constexpr int kPieceSteps = kTilePieces / 64;      // 16-byte pieces a lane stores: 6
// words between two rows of the LDS tile: 28, not 24.  A lane writes its row as six 16-byte pieces; such a write is served in groups
// of eight consecutive lanes and banks on (byte address / 4) mod 32.  With 24 words the eight rows of a group begin at banks 0, 24,
// 16, 8, 0, ... : two rows on every bank.  With 28 they begin at 0, 28, 24, 20, 16, 12, 8, 4: eight different four-bank slots, no
// conflict.  The 16-byte reads that follow (lane = consecutive pieces of the tile, groups of 16 lanes, 64 banks) skip the four pad
// words after every sixth piece, which leaves some groups with two lanes on one slot (2-way) where 24 words would leave none: the
// conflicts move from every write to some of the reads.  Rows stay 16-byte aligned (28 * 4 = 112 = 7 * 16).
constexpr int kLdsPitch = 28;
constexpr int kLdsTileWords = kTileRows * kLdsPitch;
constexpr uint32_t kNanHi = 0x7FF80000u;           // FLUX_CORR, FLUX_CORR_ERR: the bits of np.nan, 0x7FF8000000000000
constexpr int64_t kMaxRows = (int64_t)(((uint64_t)1 << 32) / kRowWords);   // 178 956 970, see above
constexpr int64_t kMaxTargets = (int64_t)1 << 20;
constexpr int64_t kMaxSegments = (int64_t)1 << 20;
constexpr int kLcPlanes = 5;                       // flux, flux_err, flux_background, centroid column, centroid row

// byte of a row at which each column begins, in TTYPE order
constexpr int kColOffset[kCols] = {0, 8, 12, 16, 24, 32, 40, 48, 56, 60, 64, 72, 80, 88};

using tp_fits::bswap32;
using tp_fits::fold32;

// The source of a call with typed pointers: float64 values travel as their bits (a NaN keeps payload and sign, -0.0 stays -0.0).
// Strides are in elements; a per-target stride of 0 is one vector shared by all targets.
struct Src {
	const uint64_t* time; int64_t time_stride;
	const uint64_t* timecorr; int64_t timecorr_stride;
	const int32_t* cadenceno; int64_t cadenceno_stride;
	const int32_t* pixel_quality; int64_t pixel_quality_stride;
	const uint64_t* lc; int64_t lc_plane_stride, lc_target_stride;   // value of plane p, target i, cadence t: lc[p * plane + i * target + t]
	const int32_t* quality; int64_t quality_stride;                  // null: zeros
	const uint64_t* pos_corr; int64_t pos_corr_stride;               // [target][t][2]; null: zeros
};

// the values of one row, native
struct RowValues {
	uint64_t time;
	uint32_t timecorr;        // float32 bits
	uint32_t cadenceno;
	uint64_t flux, flux_err, flux_bkg;
	uint32_t quality, pixel_quality;
	uint64_t centr1, centr2, pos_corr1, pos_corr2;
};

// the cadence a table row shows: the kept-row list, or the row itself; -1 where the list points outside [0, T) (such a row reads
// nothing and is written from zeros: the list lies in device memory and cannot be checked before the launch)
TP_RULE inline int64_t row_cadence(const int32_t* rows, int64_t r, int64_t T)
{
	const int64_t t = rows ? (int64_t)rows[r] : r;
	return (t >= 0 && t < T) ? t : -1;
}

// row of target i at cadence t from the source; t < 0: zeros.  TIMECORR becomes float32 rounded to nearest even, what numpy's
// assignment into an '>f4' field does (tp_fits::f64_to_f32_bits: overflow to inf, denormal results kept, a NaN quiet with its sign).
TP_RULE inline RowValues load_row(const Src& s, int64_t i, int64_t t)
{
	RowValues v{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	if (t < 0) return v;
	v.time = s.time[i * s.time_stride + t];
	v.timecorr = tp_fits::f64_to_f32_bits(s.timecorr[i * s.timecorr_stride + t]);
	v.cadenceno = (uint32_t)s.cadenceno[i * s.cadenceno_stride + t];
	const uint64_t* lc = s.lc + i * s.lc_target_stride + t;
	v.flux = lc[0];
	v.flux_err = lc[s.lc_plane_stride];
	v.flux_bkg = lc[2 * s.lc_plane_stride];
	v.centr1 = lc[3 * s.lc_plane_stride];
	v.centr2 = lc[4 * s.lc_plane_stride];
	v.quality = s.quality ? (uint32_t)s.quality[i * s.quality_stride + t] : 0u;
	v.pixel_quality = (uint32_t)s.pixel_quality[i * s.pixel_quality_stride + t];
	if (s.pos_corr) {
		v.pos_corr1 = s.pos_corr[i * s.pos_corr_stride + 2 * t];
		v.pos_corr2 = s.pos_corr[i * s.pos_corr_stride + 2 * t + 1];
	}
	return v;
}

TP_RULE inline uint32_t hi32(uint64_t v) { return (uint32_t)(v >> 32); }
TP_RULE inline uint32_t lo32(uint64_t v) { return (uint32_t)v; }

// the 24 words of the row as a little-endian machine stores them so that the bytes in memory are the big-endian row
TP_RULE inline void row_words(const RowValues& v, uint32_t w[kRowWords])
{
	w[0] = bswap32(hi32(v.time));       w[1] = bswap32(lo32(v.time));
	w[2] = bswap32(v.timecorr);         w[3] = bswap32(v.cadenceno);
	w[4] = bswap32(hi32(v.flux));       w[5] = bswap32(lo32(v.flux));
	w[6] = bswap32(hi32(v.flux_err));   w[7] = bswap32(lo32(v.flux_err));
	w[8] = bswap32(hi32(v.flux_bkg));   w[9] = bswap32(lo32(v.flux_bkg));
	w[10] = bswap32(kNanHi);            w[11] = 0u;
	w[12] = bswap32(kNanHi);            w[13] = 0u;
	w[14] = bswap32(v.quality);         w[15] = bswap32(v.pixel_quality);
	w[16] = bswap32(hi32(v.centr1));    w[17] = bswap32(lo32(v.centr1));
	w[18] = bswap32(hi32(v.centr2));    w[19] = bswap32(lo32(v.centr2));
	w[20] = bswap32(hi32(v.pos_corr1)); w[21] = bswap32(lo32(v.pos_corr1));
	w[22] = bswap32(hi32(v.pos_corr2)); w[23] = bswap32(lo32(v.pos_corr2));
}

// the sum of the row's 24 big-endian words from its native values (below 24 * 2^32)
TP_RULE inline uint64_t row_sum(const RowValues& v)
{
	uint64_t s = (uint64_t)hi32(v.time) + lo32(v.time);
	s += (uint64_t)v.timecorr + v.cadenceno;
	s += (uint64_t)hi32(v.flux) + lo32(v.flux);
	s += (uint64_t)hi32(v.flux_err) + lo32(v.flux_err);
	s += (uint64_t)hi32(v.flux_bkg) + lo32(v.flux_bkg);
	s += 2 * (uint64_t)kNanHi;
	s += (uint64_t)v.quality + v.pixel_quality;
	s += (uint64_t)hi32(v.centr1) + lo32(v.centr1);
	s += (uint64_t)hi32(v.centr2) + lo32(v.centr2);
	s += (uint64_t)hi32(v.pos_corr1) + lo32(v.pos_corr1);
	s += (uint64_t)hi32(v.pos_corr2) + lo32(v.pos_corr2);
	return s;
}

// rows of the data unit with its pad (whole blocks of 30 rows; the rows [n_rows, padded) are zeros), and its bytes
TP_RULE inline int64_t padded_rows(int64_t n_rows) { return (n_rows + kBlockRows - 1) / kBlockRows * kBlockRows; }
TP_RULE inline uint64_t unit_bytes(int64_t n_rows) { return (uint64_t)padded_rows(n_rows) * kRowBytes; }

// tiles of a target's unit and workgroups that hold them; the launch has blocks_per_target * n_targets workgroups
TP_RULE inline int64_t tiles_of(int64_t n_rows) { return (padded_rows(n_rows) + kTileRows - 1) / kTileRows; }
TP_RULE inline int64_t blocks_per_target(int64_t n_rows) { return (tiles_of(n_rows) + kWaves - 1) / kWaves; }

// where word `word` of row `row` of a tile lies in the wavefront's LDS tile, in dwords
TP_RULE inline int lds_index(int row, int word) { return row * kLdsPitch + word; }

// The 16-byte piece of its tile that lane `lane` stores in step `step` of kPieceSteps: the lanes of a wavefront are 64 consecutive
// pieces, 1 KiB of the data unit.  Piece q lies in row q / 6, at words 4 * (q % 6) of it, and 16 * q bytes into the tile.
struct Piece {
	int row, word;
	int64_t byte;
};
TP_RULE inline Piece piece_of(int lane, int step)
{
	const int q = lane + 64 * step;
	return Piece{q / kRowPieces, 4 * (q % kRowPieces), (int64_t)16 * q};
}

// ---- refusals of tp_lc_table_pack -------------------------------------------------------------------------------------------------
// the message of the first rule a call breaks, or null.  Addresses travel as integers; `offsets` is host memory.
inline const char* ranges_check(const uint64_t* offsets, const uint64_t* lengths, uint64_t length_all, int64_t n, uint64_t capacity, const char* leaves, const char* overlap)
{
	std::vector<std::pair<uint64_t, uint64_t>> spans;
	for (int64_t i = 0; i < n; i++) {
		const uint64_t len = lengths ? lengths[i] : length_all;
		if (offsets[i] > capacity || len > capacity - offsets[i]) return leaves;
		if (len) spans.emplace_back(offsets[i], len);
	}
	std::sort(spans.begin(), spans.end());
	for (size_t k = 1; k < spans.size(); k++)
		if (spans[k - 1].first + spans[k - 1].second > spans[k].first) return overlap;
	return nullptr;
}

inline const char* pack_check(const Src* s, uint64_t rows_addr, int64_t n_rows, int64_t T, int64_t n_targets, uint64_t out_addr, const uint64_t* offsets,
	uint64_t out_capacity, uint64_t sum_addr)
{
	if (s == nullptr || offsets == nullptr || out_addr == 0 || sum_addr == 0) return "tp_lc_table_pack: null pointer";
	if (s->time == nullptr || s->timecorr == nullptr || s->cadenceno == nullptr || s->pixel_quality == nullptr || s->lc == nullptr) return "tp_lc_table_pack: null pointer";
	if (!(n_targets >= 1 && n_targets <= kMaxTargets)) return "tp_lc_table_pack: n_targets must lie in [1, 2^20]";
	if (!(T >= 1 && T < ((int64_t)1 << 31))) return "tp_lc_table_pack: T must lie in [1, 2^31)";
	if (!(n_rows >= 0 && n_rows <= T)) return "tp_lc_table_pack: n_rows must lie in [0, T]";
	if (n_rows > kMaxRows) return "tp_lc_table_pack: more than kMaxRows rows: the 64-bit word sum could wrap";
	if (s->time_stride < 0 || s->timecorr_stride < 0 || s->cadenceno_stride < 0 || s->pixel_quality_stride < 0 || s->lc_plane_stride < 0 || s->lc_target_stride < 0
		|| s->quality_stride < 0 || s->pos_corr_stride < 0) return "tp_lc_table_pack: a stride is negative";
	if (out_addr % 16 != 0) return "tp_lc_table_pack: d_out must be 16-byte aligned";
	if (sum_addr % 8 != 0) return "tp_lc_table_pack: d_datasum must be 8-byte aligned";
	if (rows_addr % 4 != 0) return "tp_lc_table_pack: d_rows must be 4-byte aligned";
	for (int64_t i = 0; i < n_targets; i++)
		if (offsets[i] % 16 != 0) return "tp_lc_table_pack: an output offset is no multiple of 16";
	if (blocks_per_target(n_rows) * n_targets >= ((int64_t)1 << 31)) return "tp_lc_table_pack: the launch holds fewer than 2^31 workgroups";
	return ranges_check(offsets, nullptr, unit_bytes(n_rows), n_targets, out_capacity, "tp_lc_table_pack: a target's range leaves out_capacity",
		"tp_lc_table_pack: two targets' ranges overlap");
}

// ---- tp_lc_place ------------------------------------------------------------------------------------------------------------------
// Segment k moves length[k] bytes from src_offset[k] to dst_offset[k], all multiples of 16.  The 16-byte pieces of all segments are
// numbered in call order; first[k] is the number of segment k's first piece (n_segments + 1 values), and thread g moves piece g.
inline const char* place_check(uint64_t src_addr, uint64_t src_capacity, const uint64_t* src_offsets, const uint64_t* dst_offsets, const uint64_t* lengths,
	int64_t n_segments, uint64_t dst_addr, uint64_t dst_capacity)
{
	if (!(n_segments >= 1 && n_segments <= kMaxSegments)) return "tp_lc_place: n_segments must lie in [1, 2^20]";
	if (src_addr == 0 || dst_addr == 0 || src_offsets == nullptr || dst_offsets == nullptr || lengths == nullptr) return "tp_lc_place: null pointer";
	if (src_addr % 16 != 0 || dst_addr % 16 != 0) return "tp_lc_place: d_src and d_dst must be 16-byte aligned";
	uint64_t total = 0;
	for (int64_t k = 0; k < n_segments; k++) {
		if (src_offsets[k] % 16 != 0 || dst_offsets[k] % 16 != 0 || lengths[k] % 16 != 0) return "tp_lc_place: offsets and lengths must be multiples of 16";
		if (src_offsets[k] > src_capacity || lengths[k] > src_capacity - src_offsets[k]) return "tp_lc_place: a segment leaves the source buffer";
		if (lengths[k] >= tp_fits::kMaxSumBytes || (total += lengths[k]) >= tp_fits::kMaxSumBytes) return "tp_lc_place: a call moves fewer than 2^34 bytes";
	}
	return ranges_check(dst_offsets, lengths, 0, n_segments, dst_capacity, "tp_lc_place: a segment leaves the destination buffer",
		"tp_lc_place: two destination ranges overlap");
}

// the segment that holds piece g: the last k with first[k] <= g (segments without a piece are passed over)
TP_RULE inline int64_t segment_of(const uint64_t* first, int64_t n_segments, uint64_t g)
{
	int64_t a = 0, b = n_segments;                      // first[a] <= g < first[b]
	while (b - a > 1) {
		const int64_t m = a + (b - a) / 2;
		if (first[m] <= g) a = m; else b = m;
	}
	return a;
}

} // namespace tp_lctable
