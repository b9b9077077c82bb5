// halo_rules.h -- what Halo photometry decides (halo.hip: the TV-min solver; halo_stack.hip: the frames path; halo_cubes.hip: the
// same for the time-fastest cubes of target pixel files), each rule stated once
// over plain values: the order-preserving keys and the bookkeeping of a radix pass (select_rules.h), the pixel and cadence rules of the frames path,
// the optimiser's state machine (line search, pair keeping, history slots, stopping tests, direction), and the host tables of the
// entries with their argument checks.  No device code, no HIP runtime: the kernels call these from their parallel plumbing
// (halo_dev.h), tests/hostsim/halo_rules_host.cpp composes them serially under AddressSanitizer and UBSan, and
// tests/test_halo_rules_host.py holds that to numpy and to tests/halo_common.py (lbfgs).
// (The build sets -ffp-contract=off: an expression gives the same bits here as written out in a kernel.)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "select_rules.h"

namespace tp_halo {

constexpr int kTile = 64;            // cadences per forward / backward block
constexpr int kThreads = 256;        // every block but the stat block
constexpr int kStatThreads = 1024;   // stat block: one per problem
constexpr int kKR = 20;              // keys cached in registers per stat thread (20 480 fitted cadences; the rest are re-read)
constexpr int kMaxPitch = 4096;      // pixels per problem
constexpr int kMaxChunks = kMaxPitch / 4 / kThreads;
constexpr int kMaxHistory = 16;
constexpr int kMaxTrials = 20;
constexpr double kC1 = 1e-4;
constexpr double kPairCurv = 1e-10;
constexpr int kSelTile = 64;         // cadences per select block
constexpr int kMaxStamp = 4096;      // pixels per stamp (a Halo stamp is 22 x 22)
constexpr int kGatherRows = 8;       // rows of P per gather block

enum { ST_ACTIVE = 0, ST_CONVERGED = 1, ST_CAP = 2, ST_LINESEARCH = 3, ST_DEGENERATE = 4 };

struct HaloProb {
	int64_t p_off;      // P element offset (multiple of 4)
	int64_t c_off;      // cadence offset: fit, l, fidx, sgn
	int64_t w_off;      // offset of the pitch-padded pixel arrays (theta, g, d, w, q)
	int64_t o_off;      // offset of the unpadded pixel outputs (d_w, theta in, gradient out)
	int64_t h_off;      // offset of the history S / Y: pair k at h_off + k * pitch
	int64_t part_off;   // offset of the backward partials [ntiles][pitch]
	int32_t npix, pitch, ncad, ntiles;
};

struct HaloState {
	double f, f_prev, alpha, gtd, m;
	int32_t status, iters, trials, need_grad, initial, n_pairs, newest, nf, tmed0, tmed1;
};

struct StackGeom {
	int32_t n_frames, frame_rows, frame_cols, row0, col0, height, width, n_seg, n_targets;
};

struct GatherProb {
	int64_t p_off, c_off;
	int32_t q, npix, ncad, pitch;
};

struct NormProb {
	int64_t c_off, w_off;
	int32_t q, npix, ncad, pad;
};

// the order-preserving keys and the bookkeeping of a radix pass: select_rules.h, visible here under their names
using tp_select::okey;
using tp_select::from_key;
using tp_select::fkey;
using tp_select::from_fkey;
using tp_select::RadixPass;
using tp_select::radix_begin;
using tp_select::radix_takes_part;
using tp_select::radix_digit;
using tp_select::radix_walk;
using tp_select::radix_next;

// numpy's median of nf values: the ranks (0-based, ascending) of the one or two middle values, and the median from their keys
TP_RULE inline int mid_lo(int nf) { return (nf - 1) / 2; }
TP_RULE inline int mid_hi(int nf) { return nf / 2; }
TP_RULE inline double median_of_keys(uint64_t lo, uint64_t hi, bool two) { return two ? (from_key(lo) + from_key(hi)) / 2.0 : from_key(lo); }

//--------------------------------------------------------------------------------------------------
// the frames path: pixels and cadences of a problem
//--------------------------------------------------------------------------------------------------
// nanmedian(x.astype(float64)) < minflux from the counts: n non-NaN values, c of them < minflux, a the largest of those (key),
// b the smallest of the others (key).  Odd n: the middle value is below iff c >= (n + 1) / 2.  Even n: both middle values below
// (c >= n / 2 + 1), neither (c < n / 2), or a and b themselves: numpy's (a + b) / 2 in float64.  No value: NaN, not below.
TP_RULE inline bool drop_pixel(int32_t n, int32_t c, uint32_t akey, uint32_t bkey, double minflux)
{
	if (n <= 0) return false;
	if (n & 1) return c >= (n + 1) / 2;
	if (c >= n / 2 + 1) return true;
	if (c < n / 2) return false;
	const double m = ((double)from_fkey(akey) + (double)from_fkey(bkey)) / 2.0;
	return m < minflux;
}
// a pixel value a cadence may keep: neither NaN nor infinite
TP_RULE inline bool pixel_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }
// image offset of stamp pixel p of a target (stamp st = r1, r2, c1, c2 in CCD coordinates) inside one frame
TP_RULE inline int64_t stamp_offset(const StackGeom& g, const int32_t* st, int p)
{
	return (int64_t)(st[0] - g.row0 + p / g.width) * g.frame_cols + (st[2] - g.col0 + p % g.width);
}

//--------------------------------------------------------------------------------------------------
// the optimiser's state machine.  One step evaluates the trial point w: the stat transition judges it; an accepted point gets its
// gradient and the finish transition (pair, stopping tests, next direction and first trial).
//--------------------------------------------------------------------------------------------------
TP_RULE inline void state_init(HaloState& s, int nf)
{
	s.f = s.f_prev = s.gtd = s.m = 0.0;
	s.alpha = 1.0;
	s.iters = s.trials = s.need_grad = s.n_pairs = 0;
	s.newest = -1;
	s.initial = 1;
	s.nf = nf;
	s.tmed0 = s.tmed1 = 0;
	s.status = nf < 3 ? ST_DEGENERATE : ST_ACTIVE;   // fewer than three fitted cadences: never starts
}

TP_RULE inline bool median_valid(double m) { return m > 0.0 && std::isfinite(m); }
TP_RULE inline double objective_value(double tv, double m, bool valid) { return valid ? tv / m : INFINITY; }

// s_t = sign(l_j - l_j-1) - sign(l_j+1 - l_j) from the two differences (sign(0) = 0, an end has 0 for the missing one)
TP_RULE inline float sign_term(double dp, double dn) { return (float)(((dp > 0.0) - (dp < 0.0)) - ((dn > 0.0) - (dn < 0.0))); }

enum { kStatAccept, kStatDegenerate, kStatLineSearchFailed, kStatNextTrial };
// the first point only has to be valid; a trial has to pass the Armijo test, the 20th that does not ends the problem
TP_RULE inline int stat_decide(const HaloState& st, double ft, bool valid)
{
	if (st.initial) return valid ? kStatAccept : kStatDegenerate;
	if (valid && ft <= st.f + kC1 * st.alpha * st.gtd) return kStatAccept;
	return st.trials + 1 >= kMaxTrials ? kStatLineSearchFailed : kStatNextTrial;
}
// (`so` is the stored state, `st` the copy read at the start of the step; only the fields named change)
TP_RULE inline void stat_accept(HaloState& so, const HaloState& st, double ft, double m, int t0, int t1)
{
	if (!st.initial) {
		so.f_prev = st.f;
		so.iters = st.iters + 1;
	}
	so.f = ft;
	so.m = m;
	so.tmed0 = t0;
	so.tmed1 = t1;
	so.need_grad = 1;
}
TP_RULE inline void stat_degenerate(HaloState& so) { so.status = ST_DEGENERATE; }
TP_RULE inline void stat_line_search_failed(HaloState& so, const HaloState& st)
{
	so.trials = st.trials + 1;
	so.need_grad = 0;
	so.status = ST_LINESEARCH;
}
TP_RULE inline double next_alpha(const HaloState& st) { return st.alpha * 0.5; }
TP_RULE inline void stat_next_trial(HaloState& so, const HaloState& st, double alpha)
{
	so.trials = st.trials + 1;
	so.alpha = alpha;
	so.need_grad = 0;
}

// the tile partials part(t), t < ntiles, in a fixed order: four interleaved chains (tiles t = k mod 4), then (0 + 1) + (2 + 3)
template <class F> TP_RULE inline double sum_tiles(int ntiles, F&& part)
{
	double G0 = 0.0, G1 = 0.0, G2 = 0.0, G3 = 0.0;
	int t = 0;
	for (; t + 4 <= ntiles; t += 4) {
		G0 += part(t);
		G1 += part(t + 1);
		G2 += part(t + 2);
		G3 += part(t + 3);
	}
	if (t < ntiles) G0 += part(t);
	if (t + 1 < ntiles) G1 += part(t + 1);
	if (t + 2 < ntiles) G2 += part(t + 2);
	return (G0 + G1) + (G2 + G3);
}
// pixel p of the median row: the row of the middle cadence, or the mean of the two
TP_RULE inline double median_row(const float* r0, const float* r1, bool one, int p) { return one ? (double)r0[p] : ((double)r0[p] + (double)r1[p]) * 0.5; }
// gradient with respect to w_p from G = sum_t P[t][p] s_t
TP_RULE inline double grad_w(double G, double m, double fm, double pm) { return G / m - fm * pm; }

// the pair (s, y) of an accepted step is stored if s.y > 1e-10 y.y, in the slot after the newest (a ring of H slots)
TP_RULE inline bool pair_kept(double sy, double yy) { return sy > kPairCurv * yy; }
TP_RULE inline int next_slot(int newest, int H) { return (newest + 1) % H; }
TP_RULE inline void pair_stored(int slot, int H, int& n_pairs, int& newest)
{
	newest = slot;
	n_pairs = std::min(n_pairs + 1, H);
}
// slot of pair i of n_pairs, i = 0 the oldest
TP_RULE inline int pair_slot(int newest, int n_pairs, int i, int H) { return (newest - (n_pairs - 1 - i) + H) % H; }
TP_RULE inline double gamma_of(double sy, double yy) { return sy / yy; }
// a two-loop direction that does not descend is dropped with the whole history
TP_RULE inline bool is_descent(double gtd) { return gtd < 0.0; }

// the stopping tests, in their order: after the first gradient, and after an accepted step
TP_RULE inline int stop_initial(double gmax, double gtol, int maxiter)
{
	if (gmax <= gtol) return ST_CONVERGED;
	if (maxiter <= 0) return ST_CAP;
	return ST_ACTIVE;
}
TP_RULE inline int stop_step(double f_prev, double f, double gmax, int iters, double ftol, double gtol, int maxiter)
{
	if (f_prev - f <= ftol * fmax(fmax(fabs(f_prev), fabs(f)), 1.0)) return ST_CONVERGED;
	if (gmax <= gtol) return ST_CONVERGED;
	if (iters >= maxiter) return ST_CAP;
	return ST_ACTIVE;
}

// the final transitions of the finish step: tp_halo_objective's single evaluation, a stopped problem, the next line search
TP_RULE inline void finish_objective(HaloState& so)
{
	so.status = ST_CONVERGED;
	so.need_grad = 0;
	so.initial = 0;
}
TP_RULE inline void finish_stopped(HaloState& so, int status, int n_pairs, int newest)
{
	so.status = status;
	so.need_grad = 0;
	so.initial = 0;
	so.n_pairs = n_pairs;
	so.newest = newest;
}
TP_RULE inline void finish_next_search(HaloState& so, double gtd, int n_pairs, int newest)
{
	so.alpha = 1.0;
	so.trials = 0;
	so.gtd = gtd;
	so.need_grad = 0;
	so.initial = 0;
	so.n_pairs = n_pairs;
	so.newest = newest;
}

//--------------------------------------------------------------------------------------------------
// host tables of the solver (tp_halo_tvmin, tp_halo_objective).  A check returns the message of the first rule broken, or null.
//--------------------------------------------------------------------------------------------------
inline const char* solver_check(int32_t n, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad, const void* d_P, const void* d_fit)
{
	if (!(n >= 0 && n <= (1 << 24))) return "tp_halo: bad problem count";
	if (n == 0) return nullptr;
	if (!(h_p_offset && h_npix && h_ncad && d_P && d_fit)) return "tp_halo: null pointer";
	if ((reinterpret_cast<uintptr_t>(d_P) & 15u) != 0) return "tp_halo: d_P must be 16-byte aligned";
	for (int i = 0; i < n; i++) {
		if (!(h_npix[i] >= 1 && h_npix[i] <= kMaxPitch)) return "tp_halo: npix must lie in [1, 4096]";
		if (!(h_ncad[i] >= 0)) return "tp_halo: negative ncad";
		if (!(h_p_offset[i] >= 0 && h_p_offset[i] % 4 == 0)) return "tp_halo: p_offset must be a non-negative multiple of 4";
	}
	return nullptr;
}
inline bool settings_ok(int32_t maxiter, int32_t history, double ftol, double gtol)
{
	return maxiter >= 0 && history >= 1 && history <= kMaxHistory && ftol >= 0.0 && gtol >= 0.0;
}

// where the arrays of every problem lie in the solver's workspace, and the totals
struct SolverLayout {
	std::vector<HaloProb> prob;
	int64_t c_tot = 0, w_tot = 0, o_tot = 0, part_tot = 0, tiles_tot = 0;
	int32_t max_pitch = 4;
};
inline SolverLayout solver_layout(int32_t n, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad, int32_t history)
{
	SolverLayout L;
	L.prob.resize(n);
	for (int i = 0; i < n; i++) {
		HaloProb& p = L.prob[i];
		p.npix = h_npix[i];
		p.pitch = (h_npix[i] + 3) & ~3;
		p.ncad = h_ncad[i];
		p.ntiles = (h_ncad[i] + kTile - 1) / kTile;
		p.p_off = h_p_offset[i];
		p.c_off = L.c_tot;
		p.w_off = L.w_tot;
		p.o_off = L.o_tot;
		p.h_off = L.w_tot * history;
		p.part_off = L.part_tot;
		L.c_tot += p.ncad;
		L.w_tot += p.pitch;
		L.o_tot += p.npix;
		L.part_tot += (int64_t)p.ntiles * p.pitch;
		L.tiles_tot += p.ntiles;
		L.max_pitch = std::max(L.max_pitch, p.pitch);
	}
	return L;
}
inline const char* solver_layout_check(const SolverLayout& L)
{
	return (L.tiles_tot < (int64_t)1 << 30 && L.c_tot < (int64_t)1 << 31) ? nullptr : "tp_halo: too many cadences";
}

// every step moves each active problem on by one evaluation; an iteration is at most 1 + kMaxTrials of them
inline int64_t max_steps(int objective, int32_t maxiter) { return objective ? 1 : ((int64_t)maxiter + 1) * (kMaxTrials + 1) + 1; }
// steps between two looks at the states: 4, 8, 16, 32, 32, ...
inline int32_t first_poll(int objective) { return objective ? 1 : 4; }
inline int32_t next_poll(int32_t poll) { return std::min(poll * 2, 32); }

// the launch lists over the problems still active (states null: over all): plist the problems, list2 their (problem, tile) pairs
inline void launch_lists(const std::vector<HaloProb>& prob, const HaloState* states, std::vector<int32_t>& list2, std::vector<int32_t>& plist)
{
	list2.clear();
	plist.clear();
	for (int i = 0; i < (int)prob.size(); i++) {
		if (states && states[i].status != ST_ACTIVE) continue;
		plist.push_back(i);
		for (int t = 0; t < prob[i].ntiles; t++) {
			list2.push_back(i);
			list2.push_back(t);
		}
	}
}

//--------------------------------------------------------------------------------------------------
// host tables of the frames path (tp_halo_select_stack, tp_halo_gather_stack, tp_halo_outputs_stack)
//--------------------------------------------------------------------------------------------------
inline const char* stack_check(const StackGeom& g, const void* d_stack, const int32_t* h_stamps)
{
	if (!(d_stack && h_stamps)) return "tp_halo: null pointer";
	if (!(g.n_frames >= 1 && g.frame_rows >= 1 && g.frame_cols >= 1 && g.n_targets >= 1 && g.n_targets <= 65535)) return "tp_halo: bad stack or batch size";
	if (!(g.height >= 1 && g.width >= 1 && (int64_t)g.height * g.width <= kMaxStamp)) return "tp_halo: a stamp holds 1 .. 4096 pixels";
	if (!(g.n_seg >= 1 && g.n_seg <= 64)) return "tp_halo: 1 .. 64 segments";
	for (int i = 0; i < g.n_targets; i++) {
		const int32_t* s = h_stamps + 4 * i;
		if (!(s[1] - s[0] == g.height && s[3] - s[2] == g.width)) return "tp_halo: every stamp of a call has the call's height and width";
		if (!(s[0] >= g.row0 && s[1] <= g.row0 + g.frame_rows && s[2] >= g.col0 && s[3] <= g.col0 + g.frame_cols)) return "tp_halo: stamp outside the frame stack";
	}
	return nullptr;
}
inline const char* seg_check(const StackGeom& g, const int32_t* h_seg)
{
	if (!h_seg) return "tp_halo: null pointer";
	int32_t mx = -1;
	for (int t = 0; t < g.n_frames; t++) {
		if (!(h_seg[t] >= -1)) return "tp_halo: segment below -1";
		mx = std::max(mx, h_seg[t]);
	}
	return mx + 1 == g.n_seg ? nullptr : "tp_halo: n_seg must be the largest segment plus one";
}

// the cadences of every segment in ascending order (cadlist; segment k from seg_off[k]), their fit flags, and the tiles of kSelTile
// of them: (segment, first, one past the last entry of cadlist)
struct SegLists {
	std::vector<int32_t> cadlist, seg_off, tiles;
	std::vector<uint8_t> fitlist;
};
inline SegLists seg_lists(int32_t n_frames, int32_t n_seg, const int32_t* h_seg, const int32_t* h_quality, int32_t bitmask)
{
	SegLists s;
	s.seg_off.assign(n_seg + 1, 0);
	for (int k = 0; k < n_seg; k++) {
		for (int t = 0; t < n_frames; t++)
			if (h_seg[t] == k) {
				s.cadlist.push_back(t);
				s.fitlist.push_back((h_quality[t] & bitmask) == 0);
			}
		s.seg_off[k + 1] = (int32_t)s.cadlist.size();
		for (int j = s.seg_off[k]; j < s.seg_off[k + 1]; j += kSelTile) {
			s.tiles.push_back(k);
			s.tiles.push_back(j);
			s.tiles.push_back(std::min(j + kSelTile, s.seg_off[k + 1]));
		}
	}
	return s;
}

// the problems a gather call packs; `max_ncad` the longest of them
inline const char* gather_table(const StackGeom& g, int32_t n_run, const int32_t* h_index, const int64_t* h_p_offset, const int32_t* h_npix,
	const int32_t* h_ncad, std::vector<GatherProb>& probs, int32_t& max_ncad)
{
	const int HW = g.height * g.width;
	probs.resize(n_run);
	int64_t c_tot = 0;
	max_ncad = 0;
	for (int r = 0; r < n_run; r++) {
		if (!(h_index[r] >= 0 && h_index[r] < (int64_t)g.n_targets * g.n_seg)) return "tp_halo_gather_stack: problem index out of range";
		if (!(h_npix[r] >= 1 && h_npix[r] <= HW && h_ncad[r] >= 0 && h_ncad[r] <= g.n_frames)) return "tp_halo_gather_stack: npix or ncad out of range";
		if (!(h_p_offset[r] >= 0 && h_p_offset[r] % 4 == 0)) return "tp_halo_gather_stack: p_offset must be a non-negative multiple of 4";
		probs[r] = GatherProb{h_p_offset[r], c_tot, h_index[r], h_npix[r], h_ncad[r], (h_npix[r] + 3) & ~3};
		c_tot += h_ncad[r];
		max_ncad = std::max(max_ncad, h_ncad[r]);
	}
	return nullptr;
}

// the problems the outputs are formed from (at least one entry, for the upload), and for every problem q its place among them or -1
inline const char* norm_table(const StackGeom& g, int32_t n_run, const int32_t* h_index, const int32_t* h_npix, const int32_t* h_ncad,
	std::vector<NormProb>& probs, std::vector<int32_t>& run)
{
	const int HW = g.height * g.width;
	const int64_t n_prob = (int64_t)g.n_targets * g.n_seg;
	probs.assign(std::max(n_run, 1), NormProb{});
	run.assign(n_prob, -1);
	int64_t c_tot = 0, w_tot = 0;
	for (int r = 0; r < n_run; r++) {
		if (!(h_index[r] >= 0 && h_index[r] < n_prob && run[h_index[r]] < 0)) return "tp_halo_outputs_stack: bad problem index";
		if (!(h_npix[r] >= 1 && h_npix[r] <= HW && h_ncad[r] >= 0 && h_ncad[r] <= g.n_frames)) return "tp_halo_outputs_stack: npix or ncad out of range";
		probs[r] = NormProb{c_tot, w_tot, h_index[r], h_npix[r], h_ncad[r], 0};
		run[h_index[r]] = r;
		c_tot += h_ncad[r];
		w_tot += h_npix[r];
	}
	return nullptr;
}

//--------------------------------------------------------------------------------------------------
// host tables of the cubes path (tp_halo_select_cubes, tp_halo_gather_cubes, tp_halo_outputs_cubes): a group of target pixel files in
// one time-fastest cube [n_targets][height * width][t_pitch].  Every target has its own segments: problem q = h_prob_off[i] + k is
// segment k of target i, n_prob = h_prob_off[n_targets].
//--------------------------------------------------------------------------------------------------
struct CubeGeom {
	int32_t n_targets, height, width, n_cad, t_pitch, n_prob;
};
// first element of the series of stamp pixel p of target i
TP_RULE inline int64_t cube_offset(const CubeGeom& g, int i, int p) { return ((int64_t)i * (g.height * g.width) + p) * g.t_pitch; }
// target of problem q (h_prob_off rises: the last i with h_prob_off[i] <= q)
inline int32_t cube_target_of(const int32_t* h_prob_off, int32_t n_targets, int32_t q)
{
	return (int32_t)(std::upper_bound(h_prob_off, h_prob_off + n_targets + 1, q) - h_prob_off) - 1;
}

// the geometry and the problem offsets; sets g.n_prob
inline const char* check_cube(CubeGeom& g, const void* d_cube, const int32_t* h_prob_off)
{
	g.n_prob = 0;
	if (!(d_cube && h_prob_off)) return "tp_halo: null pointer";
	if (!(g.n_targets >= 1 && g.n_targets <= 65535 && g.n_cad >= 1 && g.t_pitch >= g.n_cad)) return "tp_halo: bad cube or batch size";
	if (!(g.height >= 1 && g.width >= 1 && (int64_t)g.height * g.width <= kMaxStamp)) return "tp_halo: a stamp holds 1 .. 4096 pixels";
	if (h_prob_off[0] != 0) return "tp_halo: h_prob_off must start at 0";
	for (int i = 0; i < g.n_targets; i++) {
		const int64_t n_seg = (int64_t)h_prob_off[i + 1] - h_prob_off[i];
		if (!(n_seg >= 1 && n_seg <= 64)) return "tp_halo: h_prob_off must rise by 1 .. 64 segments per target";
	}
	if (!(h_prob_off[g.n_targets] <= 65535)) return "tp_halo: at most 65535 problems per call";
	g.n_prob = h_prob_off[g.n_targets];
	return nullptr;
}
// h_seg [n_targets][n_cad]: -1 .. n_seg_i - 1 in row i
inline const char* check_cube_seg(const CubeGeom& g, const int32_t* h_prob_off, const int32_t* h_seg)
{
	if (!h_seg) return "tp_halo: null pointer";
	for (int i = 0; i < g.n_targets; i++) {
		const int32_t n_seg = h_prob_off[i + 1] - h_prob_off[i];
		const int32_t* s = h_seg + (int64_t)i * g.n_cad;
		for (int t = 0; t < g.n_cad; t++)
			if (!(s[t] >= -1 && s[t] < n_seg)) return "tp_halo: segment outside -1 .. n_seg - 1 of its target";
	}
	return nullptr;
}

// per target the cadences with a segment, sorted by (segment, cadence), in row i of cadlist [n_targets][n_cad] with their fit flags;
// problem q owns the entries [lo[q], hi[q]) of its target's row; target[q] is that target
struct CubeLists {
	std::vector<int32_t> cadlist, lo, hi, target;
	std::vector<uint8_t> fitlist;
};
inline CubeLists cube_lists(const CubeGeom& g, const int32_t* h_prob_off, const int32_t* h_seg, const int32_t* h_quality, int32_t bitmask)
{
	CubeLists s;
	const int T = g.n_cad;
	s.cadlist.assign((size_t)g.n_targets * T, 0);
	s.fitlist.assign((size_t)g.n_targets * T, 0);
	s.lo.assign(g.n_prob, 0);
	s.hi.assign(g.n_prob, 0);
	s.target.assign(g.n_prob, 0);
	for (int i = 0; i < g.n_targets; i++) {
		const int32_t q0 = h_prob_off[i], n_seg = h_prob_off[i + 1] - q0;
		const int32_t* seg = h_seg + (int64_t)i * T;
		const int32_t* quality = h_quality + (int64_t)i * T;
		int32_t count[64] = {0};
		for (int t = 0; t < T; t++)
			if (seg[t] >= 0) count[seg[t]]++;
		int32_t at = 0, next[64] = {0};
		for (int k = 0; k < n_seg; k++) {
			s.target[q0 + k] = i;
			s.lo[q0 + k] = next[k] = at;
			at += count[k];
			s.hi[q0 + k] = at;
		}
		for (int t = 0; t < T; t++)
			if (seg[t] >= 0) {
				const int64_t j = (int64_t)i * T + next[seg[t]]++;
				s.cadlist[j] = t;
				s.fitlist[j] = (quality[t] & bitmask) == 0;
			}
	}
	return s;
}

// the problems a gather / outputs call of the cubes path works on: the stack's tables over n_prob problems of n_cad cadences
inline StackGeom cube_as_problems(const CubeGeom& g) { return StackGeom{g.n_cad, 1, 1, 0, 0, g.height, g.width, 1, g.n_prob}; }
inline const char* check_cube_gather(const CubeGeom& g, int32_t n_run, const int32_t* h_index, const int64_t* h_p_offset, const int32_t* h_npix,
	const int32_t* h_ncad, std::vector<GatherProb>& probs, int32_t& max_ncad, int32_t& max_pitch)
{
	const char* bad = gather_table(cube_as_problems(g), n_run, h_index, h_p_offset, h_npix, h_ncad, probs, max_ncad);
	max_pitch = 0;
	if (!bad)
		for (const GatherProb& p : probs) max_pitch = std::max(max_pitch, p.pitch);
	return bad ? "tp_halo_gather_cubes: problem index, npix, ncad or p_offset out of range" : nullptr;
}
inline const char* check_cube_norm(const CubeGeom& g, int32_t n_run, const int32_t* h_index, const int32_t* h_npix, const int32_t* h_ncad,
	std::vector<NormProb>& probs, std::vector<int32_t>& run)
{
	return norm_table(cube_as_problems(g), n_run, h_index, h_npix, h_ncad, probs, run) ? "tp_halo_outputs_cubes: problem index, npix or ncad out of range" : nullptr;
}

} // namespace tp_halo
