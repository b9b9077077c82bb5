// starpos_rules.h -- what the per-target star positions decide (starpos.hip, tp_star_positions_targets), each rule stated once over
// plain values: the argument checks, the grid -- which cadence a thread owns and which stars a block walks --, the row of a target's
// shift series a cadence reads (the lookup), the float32 narrowing of the shift, the float32 sum and its widening, and where every
// value lies.  No device code, no HIP runtime: the kernel calls these from its parallel plumbing, tests/hostsim/starpos_host.cpp
// composes them serially into complete position arrays under AddressSanitizer and UBSan, and tests/test_tpf_linpsf_host.py holds
// that to numpy bit for bit.
#pragma once
#include <cstdint>

#ifndef TP_RULE
#if defined(__HIPCC__)
#define TP_RULE __host__ __device__
#else
#define TP_RULE
#endif
#endif

namespace tp_starpos {

constexpr int kThreads = 256;             // a workgroup: 256 consecutive cadences of one star at a time
constexpr int64_t kMaxGridY = 65535;      // gridDim.y: a block walks the stars blockIdx.y, blockIdx.y + gridDim.y, ...
constexpr int64_t kMaxValues = ((int64_t)1 << 60);   // values of d_pos, d_shift or d_lookup: byte offsets stay inside int64

// the message of the first rule the sizes of a call break, or null
inline const char* sizes_check(int64_t n_stars, int64_t n_cad, int64_t n_targets, int64_t shift_pitch, bool has_lookup, int64_t lookup_pitch, int64_t pos_pitch)
{
	if (!(n_stars >= 0 && n_cad >= 0 && n_targets >= 0)) return "tp_star_positions_targets: bad sizes";
	if (!(pos_pitch >= n_cad)) return "tp_star_positions_targets: pos_pitch must be at least n_cad";
	if (n_stars == 0 || n_cad == 0) return nullptr;
	if (!(n_targets >= 1)) return "tp_star_positions_targets: stars without a target";
	if (has_lookup) {
		if (!(lookup_pitch >= n_cad)) return "tp_star_positions_targets: lookup_pitch must be at least n_cad";
		if (!(shift_pitch >= 1)) return "tp_star_positions_targets: shift_pitch must be at least 1";
	} else if (!(shift_pitch >= n_cad)) return "tp_star_positions_targets: shift_pitch must be at least n_cad without a lookup";
	if (!(n_stars <= kMaxValues / pos_pitch && n_targets <= kMaxValues / shift_pitch && (!has_lookup || n_targets <= kMaxValues / lookup_pitch)))
		return "tp_star_positions_targets: too many values for 64-bit offsets";
	return nullptr;
}

// the pointers of a call that has work to do (addresses travel as integers; d_lookup may be null: identity)
inline const char* pointers_check(uint64_t base_addr, uint64_t star_target_addr, uint64_t shift_addr, uint64_t pos_addr)
{
	if (base_addr == 0 || star_target_addr == 0 || shift_addr == 0 || pos_addr == 0) return "tp_star_positions_targets: null pointer";
	return nullptr;
}

// the grid: x over the cadences, y over the stars
TP_RULE inline int64_t blocks_x(int64_t n_cad) { return (n_cad + kThreads - 1) / kThreads; }
TP_RULE inline int64_t blocks_y(int64_t n_stars) { return n_stars < kMaxGridY ? n_stars : kMaxGridY; }
TP_RULE inline int64_t cadence_of(int64_t block_x, int thread) { return block_x * kThreads + thread; }

// where the values lie, in elements
TP_RULE inline int64_t shift_index(int64_t target, int64_t row, int64_t shift_pitch) { return target * shift_pitch + row; }
TP_RULE inline int64_t lookup_index(int64_t target, int64_t k, int64_t lookup_pitch) { return target * lookup_pitch + k; }
TP_RULE inline int64_t pos_index(int64_t star, int64_t k, int64_t pos_pitch) { return star * pos_pitch + k; }

// A star names its target and a lookup names a row of that target's series.  Both are data on the device that no host check has
// seen: a value outside its array is never followed, the position is NaN.
TP_RULE inline bool target_ok(int64_t target, int64_t n_targets) { return target >= 0 && target < n_targets; }
TP_RULE inline bool row_ok(int64_t row, int64_t shift_pitch) { return row >= 0 && row < shift_pitch; }

// the row of the shift series cadence k reads: the lookup's, or k itself (the plugin's argmin(|tref - tref[k]|) of a finite, strictly
// increasing tref)
TP_RULE inline int64_t cadence_row(const int32_t* lookup, int64_t target, int64_t k, int64_t lookup_pitch)
{
	return lookup ? (int64_t)lookup[lookup_index(target, k, lookup_pitch)] : k;
}

// catalog_attime: `cat['row_stamp'] + np.float32(jit[k, 1])` -- the float64 POS_CORR value narrowed to float32, added to the float32
// stamp coordinate in float32 -- and do_photometry's widening of the sum into its float64 position array.  A NaN shift stays NaN.
TP_RULE inline float narrow(double shift) { return (float)shift; }
TP_RULE inline float moved(float base, float shift) { return base + shift; }
TP_RULE inline double widen(float sum) { return (double)sum; }
TP_RULE inline double position(float base, double shift) { return widen(moved(base, narrow(shift))); }
TP_RULE inline double no_position() { return __builtin_nan(""); }

// position of star s at cadence k, every read behind its bounds rule
TP_RULE inline double star_position(const float* base, const int32_t* star_target, const double* shift, int64_t shift_pitch, const int32_t* lookup,
	int64_t lookup_pitch, int64_t n_targets, int64_t s, int64_t k)
{
	const int64_t target = star_target[s];
	if (!target_ok(target, n_targets)) return no_position();
	const int64_t row = cadence_row(lookup, target, k, lookup_pitch);
	if (!row_ok(row, shift_pitch)) return no_position();
	return position(base[s], shift[shift_index(target, row, shift_pitch)]);
}

} // namespace tp_starpos
