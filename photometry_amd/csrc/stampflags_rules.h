// stampflags_rules.h -- what the per-stamp flag series decides (stampflags.hip), each rule stated once over plain values: the argument
// checks of tp_stamp_flag_series (the stamps among them), a stamp relative to the frames, the grid -- which frames and which target
// a wavefront owns --, which pixel of a stamp a lane reads in which step, where that pixel lies in the stack, and what is stored.
// No device code, no HIP runtime: the kernel calls these from its parallel plumbing, tests/hostsim/stampflags_rules_host.cpp
// composes them serially into a complete series under AddressSanitizer and UBSan, and tests/test_stampflags_host.py holds that to numpy.
#pragma once
#include <cstdint>

#ifndef TP_RULE
#if defined(__HIPCC__)
#define TP_RULE __host__ __device__
#else
#define TP_RULE
#endif
#endif

namespace tp_sflags {

constexpr int kThreads = 256;     // a workgroup: four wavefronts, one target each
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kTileT = 16;        // frames a wavefront walks for its target: 16 int32 results, one 64-byte run of the target's row
constexpr int kLaneCols = 16;     // a wavefront lies over a stamp as 4 rows x 16 columns: 16 consecutive bytes of a stamp row per row of lanes
constexpr int kLaneRows = kWave / kLaneCols;
constexpr int64_t kMaxBlocks = ((int64_t)1 << 31) - 1;   // blockIdx.x
constexpr int64_t kMaxFrame = ((int64_t)1 << 31) - 1;    // rows x columns of a frame: pixel offsets inside a frame travel as int32

// a stamp relative to the frames: rows [r1, r2), columns [c1, c2) of a frame; the stamp of a target without one is empty (all 0)
struct RelStamp {
	int32_t r1, r2, c1, c2;
};

TP_RULE inline bool no_stamp(const int64_t* s) { return s[0] == -1 && s[1] == -1 && s[2] == -1 && s[3] == -1; }

// the message of the first rule a stamp (r1, r2, c1, c2 in CCD pixels) breaks, or null
inline const char* stamp_check(const int64_t* s, int64_t frame_rows, int64_t frame_cols, int64_t row0, int64_t col0)
{
	if (no_stamp(s)) return nullptr;
	if (!(s[1] > s[0] && s[3] > s[2])) return "tp_stamp_flag_series: a stamp is empty or reversed";
	if (!(s[0] >= row0 && s[1] <= row0 + frame_rows && s[2] >= col0 && s[3] <= col0 + frame_cols)) return "tp_stamp_flag_series: a stamp leaves the frames";
	return nullptr;
}

TP_RULE inline int64_t tiles_t(int64_t n_frames) { return (n_frames + kTileT - 1) / kTileT; }
TP_RULE inline int64_t groups_n(int64_t n_targets) { return (n_targets + kWaves - 1) / kWaves; }

// the message of the first rule a call breaks, or null.  Addresses travel as integers; `stamps` is host memory.
inline const char* series_check(uint64_t flags_addr, int64_t n_frames, int64_t frame_rows, int64_t frame_cols, int64_t frame_stride, int64_t row0, int64_t col0,
	int64_t n_targets, const int64_t* stamps, uint32_t flag_mask, uint64_t out_addr, int64_t out_pitch)
{
	if (flags_addr == 0 || stamps == nullptr || out_addr == 0) return "tp_stamp_flag_series: null pointer";
	if (out_addr % 4 != 0) return "tp_stamp_flag_series: d_out must be 4-byte aligned";
	if (flag_mask == 0) return "tp_stamp_flag_series: flag_mask must not be zero";
	if (!(n_frames >= 1)) return "tp_stamp_flag_series: n_frames must be at least 1";
	if (!(n_targets >= 1)) return "tp_stamp_flag_series: n_targets must be at least 1";
	if (!(frame_rows >= 1 && frame_cols >= 1 && frame_rows * frame_cols <= kMaxFrame)) return "tp_stamp_flag_series: a frame holds between 1 and 2^31 - 1 pixels";
	if (!(frame_stride >= frame_rows * frame_cols)) return "tp_stamp_flag_series: frame_stride must be at least frame_rows * frame_cols";
	if (!(out_pitch >= n_frames)) return "tp_stamp_flag_series: out_pitch must be at least n_frames";
	if (!(tiles_t(n_frames) <= kMaxBlocks / groups_n(n_targets))) return "tp_stamp_flag_series: too many (target, frame) pairs for one launch";
	for (int64_t i = 0; i < n_targets; i++)
		if (const char* msg = stamp_check(stamps + 4 * i, frame_rows, frame_cols, row0, col0)) return msg;
	return nullptr;
}

// a checked stamp relative to the frames
inline RelStamp relative(const int64_t* s, int64_t row0, int64_t col0)
{
	if (no_stamp(s)) return RelStamp{0, 0, 0, 0};
	return RelStamp{(int32_t)(s[0] - row0), (int32_t)(s[1] - row0), (int32_t)(s[2] - col0), (int32_t)(s[3] - col0)};
}

// Block `block` of the grid: the targets vary fastest, so the workgroups in flight at one time read the same few frames (a frame
// comes out of HBM once and every stamp on it finds its lines in cache).  Wavefront `wave` of the block owns one target.
TP_RULE inline int64_t block_tile(int64_t block, int64_t n_groups) { return block / n_groups; }
TP_RULE inline int64_t block_target(int64_t block, int64_t n_groups, int wave) { return (block % n_groups) * kWaves + wave; }
TP_RULE inline int64_t grid_blocks(int64_t n_frames, int64_t n_targets) { return tiles_t(n_frames) * groups_n(n_targets); }

// The pixel of the stamp lane `lane` reads in step (row_step, col_step): rows go by kLaneRows, columns by kLaneCols.
TP_RULE inline int32_t lane_row(const RelStamp& s, int lane, int32_t row_step) { return s.r1 + row_step * kLaneRows + lane / kLaneCols; }
TP_RULE inline int32_t lane_col(const RelStamp& s, int lane, int32_t col_step) { return s.c1 + col_step * kLaneCols + lane % kLaneCols; }
TP_RULE inline int32_t row_steps(const RelStamp& s) { return (s.r2 - s.r1 + kLaneRows - 1) / kLaneRows; }
TP_RULE inline int32_t col_steps(const RelStamp& s) { return (s.c2 - s.c1 + kLaneCols - 1) / kLaneCols; }
TP_RULE inline bool in_stamp(const RelStamp& s, int32_t row, int32_t col) { return row < s.r2 && col < s.c2; }

// byte of the stack that holds pixel (row, col) of frame t
TP_RULE inline int64_t flag_byte(int64_t t, int64_t frame_stride, int32_t frame_cols, int32_t row, int32_t col) { return t * frame_stride + (int64_t)row * frame_cols + col; }
TP_RULE inline bool flagged(uint8_t value, uint32_t flag_mask) { return ((uint32_t)value & flag_mask) != 0; }
// value of the output [n_targets][out_pitch] that holds frame t of target i; only t < n_frames is ever stored
TP_RULE inline int64_t out_index(int64_t target, int64_t t, int64_t out_pitch) { return target * out_pitch + t; }
TP_RULE inline int32_t out_of(bool any, int32_t out_value) { return any ? out_value : 0; }

} // namespace tp_sflags
