// aperture_dev.h -- device code of A6 shared by the stand-alone extraction kernels (aperture.hip) and the fused
// per-target kernel (fused.hip).  See aperture.hip for the arithmetic contract and its reference citations.
#pragma once
#include "common.h"
#include <cmath>

namespace tp_ap {

constexpr int kMaxList = 128;      // small kernel: mask pixels held in LDS
constexpr int kChunk = 1024;       // big kernel: ordered mask pixels staged per round
constexpr int kMaxLeaves = 4096;   // big kernel: pairwise leaves (each 65..128 pixels)
constexpr int kMaxDepth = 24;

template <int VEC> struct Vec;
template <> struct Vec<4> {
	static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
		float4 t = *reinterpret_cast<const float4*>(p);
		v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
	}
};
template <> struct Vec<2> {
	static __device__ __forceinline__ void load(const float* p, float (&v)[2]) {
		float2 t = *reinterpret_cast<const float2*>(p);
		v[0] = t.x; v[1] = t.y;
	}
};
template <> struct Vec<1> {
	static __device__ __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = *p; }
};

// Per-thread state for VEC cadences
template <int VEC>
struct CadState {
	float r[VEC][8];      // pairwise accumulators: flux
	float e[VEC][8];      // pairwise accumulators: err^2
	float bk[VEC][8];     // pairwise accumulators: background (NaN -> 0, np.nansum)
	float fres[VEC], eres[VEC], bres[VEC];
	double cw[VEC], ccol[VEC], crow[VEC];
	bool f_allnan[VEC], f_allzero[VEC], b_allnan[VEC];

	__device__ __forceinline__ void init() {
#pragma unroll
		for (int c = 0; c < VEC; c++) {
			fres[c] = 0.f; eres[c] = 0.f; bres[c] = 0.f;
			cw[c] = 0.0; ccol[c] = 0.0; crow[c] = 0.0;
			f_allnan[c] = true; f_allzero[c] = true; b_allnan[c] = true;
		}
	}
	// everything except the pairwise flux / err / background sums
	__device__ __forceinline__ void side(const float (&v)[VEC], double col, double row) {
#pragma unroll
		for (int c = 0; c < VEC; c++) {
			const float x = v[c];
			f_allnan[c] = f_allnan[c] && (x != x);
			f_allzero[c] = f_allzero[c] && (x == 0.f);
			// (branch-free: a value that is not positive enters as +0.0, which changes none of the three sums)
			const double w = (x > 0.f) ? (double)x : 0.0;
			cw[c] += w;
			ccol[c] += col * w;
			crow[c] += row * w;
		}
	}
	// np.nansum (photometry.py:201) = np.sum of the values with NaN replaced by 0: the term that enters the pairwise tree
	__device__ __forceinline__ void bkg_terms(const float (&b)[VEC], float (&y)[VEC]) {
#pragma unroll
		for (int c = 0; c < VEC; c++) {
			const bool fin = (b[c] == b[c]);
			b_allnan[c] = b_allnan[c] && !fin;
			y[c] = fin ? b[c] : 0.f;
		}
	}
};

__device__ __forceinline__ float combine8(const float (&r)[8]) {
	return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

struct Args {
	const float* images; const float* images_err; const float* backgrounds;
	int32_t bkg_mode; int64_t bkg_series_pitch;   // 0 cube, 1 series per target, 2 no background (aperture-only)
	const float* subtract; int64_t subtract_pitch;
	const uint8_t* mask; const int32_t* stamps; const int32_t* status;
	double* flux; double* flux_err; double* flux_bkg; double* ccol; double* crow;
	int64_t out_pitch; int n_cad; int height; int width; int64_t t_pitch; int n_targets;
	// optional work list of the big-mask kernel: big_list[0] = count, big_list[1..] = targets (filled by the fused kernel)
	int32_t* big_list;
	// STACK mode (stack_cols > 0; tp_aperture_extract_stack): images / images_err / backgrounds are not per-target cubes but the
	// TIME-MAJOR stacks of a CCD region, [stack rows x stack_cols][t_pitch] (tp_frames_transpose): pixel (r, c) of a target's stamp
	// is the stack's row (stamps[4 t] - stack_row0 + r) * stack_cols + stamps[4 t + 2] - stack_col0 + c.  Nothing is cut.
	int32_t stack_cols = 0, stack_row0 = 0, stack_col0 = 0;
};

// where the time series of the pixels of `target` start (cube mode: its cube; stack mode: the stack) and which row of it holds
// stamp pixel p = pr * width + pc
__device__ __forceinline__ int64_t target_base(const Args& a, int target, int P) { return a.stack_cols ? 0 : (int64_t)target * P * a.t_pitch; }
__device__ __forceinline__ int stack_origin(const Args& a, int target) {
	return a.stack_cols ? ((a.stamps[target * 4 + 0] - a.stack_row0) * a.stack_cols + (a.stamps[target * 4 + 2] - a.stack_col0)) : 0;
}
__device__ __forceinline__ int pixel_row(const Args& a, int origin, int p, int pr, int pc) { return a.stack_cols ? (origin + pr * a.stack_cols + pc) : p; }

template <int VEC, class State>
__device__ __forceinline__ void store_outputs(const Args& a, int target, int k0, const State& st, int M) {
	const int64_t ob = (int64_t)target * a.out_pitch;
	const double nan = __builtin_nan("");
#pragma unroll
	for (int c = 0; c < VEC; c++) {
		const int k = k0 + c;
		if (k >= a.n_cad) continue;
		const bool bad = (M == 0) || st.f_allnan[c] || st.f_allzero[c];
		a.flux[ob + k] = bad ? nan : (double)st.fres[c];
		a.flux_err[ob + k] = bad ? nan : (double)sqrtf(st.eres[c]);
		const bool haspos = st.cw[c] > 0.0;
		a.ccol[ob + k] = (bad || !haspos) ? nan : st.ccol[c] / st.cw[c];
		a.crow[ob + k] = (bad || !haspos) ? nan : st.crow[c] / st.cw[c];
		if (a.flux_bkg) a.flux_bkg[ob + k] = (M == 0 || a.bkg_mode == 2 || st.b_allnan[c]) ? nan : (double)st.bres[c];
	}
}

// Ordered (raster) compaction of the next mask pixels starting at *p_next into list[0..cap), by
// ONE wavefront.  Returns the number stored; advances *p_next.  With count_rest, keeps counting
// (without storing) to the end of the mask and returns the total in *total.
__device__ __forceinline__ int compact_mask(const uint8_t* m, int P, int& p_next, int* list, int cap, int lane,
	bool count_rest, int* total)
{
	int n = 0;
	int p0 = p_next;
	for (; p0 < P; p0 += 64) {
		const int p = p0 + lane;
		const bool in = (p < P) && (m[p] != 0);
		const unsigned long long bal = __ballot(in);
		const int pos = n + __popcll(bal & ((1ull << lane) - 1ull));
		const int cnt = __popcll(bal);
		if (n + cnt > cap) {
			if (!count_rest) {
				// store only what fits, stop *inside* this group: find the pixel where the list fills
				if (in && pos < cap) list[pos] = p;
				// p_next = index of the first pixel NOT stored
				const unsigned long long notstored = __ballot(in && pos >= cap);
				p_next = p0 + (int)__ffsll((long long)notstored) - 1;
				return cap;
			}
			if (in && pos < cap) list[pos] = p;
			n += cnt;
			continue;
		}
		if (in && pos < cap) list[pos] = p;
		n += cnt;
	}
	p_next = P;
	if (total) *total = n;
	return n < cap ? n : cap;
}

// The pixel list of the stand-alone small-mask extraction carries a pixel's row beside its index (index in the low, row in the high 16
// bits; a stamp holds at most 65 535 pixels): the extraction turns every list entry into (row, column) once per cadence block,
// and a division by the run-time stamp width is ~30 instructions -- a third of the vector work of a pixel (lab clocks, round 4).
__device__ __forceinline__ void pack_rows(int* list, int M, int width, int lane, int nlanes) {
	for (int i = lane; i < M; i += nlanes) { const int p = list[i]; list[i] = p | ((p / width) << 16); }
}

// Extraction of the cadences q_first, q_first + q_stride, ... (VEC cadences each) of one target with a mask of
// M <= kMaxList pixels listed (raster order) in s_list: a single pairwise leaf.
template <int VEC>
__device__ __forceinline__ void extract_small(const Args& a, int target, const int* s_list, int M, int q_first, int q_stride)
{
	const int P = a.height * a.width;
	const int col0 = a.stamps[target * 4 + 2] + 1; // 1-based CCD column of stamp column 0
	const int row0 = a.stamps[target * 4 + 0] + 1;
	const int64_t tb = target_base(a, target, P);
	const int origin = stack_origin(a, target);
	const float* img = a.images + tb;
	const float* err = a.images_err + tb;
	const float* bkg = (a.bkg_mode == 0) ? (a.backgrounds + tb) : (a.backgrounds + (int64_t)target * a.bkg_series_pitch);
	const bool has_bkg = (a.bkg_mode != 2);
	const int nq = (a.n_cad + VEC - 1) / VEC;
	const int nblk = M - (M & 7);

	for (int q = q_first; q < nq; q += q_stride) {
		const int k0 = q * VEC;
		CadState<VEC> st;
		st.init();
		float bser[VEC], ssub[VEC];
		if (a.bkg_mode == 1) Vec<VEC>::load(bkg + k0, bser);
		if (a.subtract) Vec<VEC>::load(a.subtract + (int64_t)target * a.subtract_pitch + k0, ssub);

		auto fetch = [&](int idx, float (&v)[VEC], float (&e2)[VEC], float (&y)[VEC]) {
			const int pk = s_list[idx];
			const int p = pk & 0xffff;
			const int pr = (int)((unsigned)pk >> 16);
			const int pc = p - pr * a.width;
			const int64_t off = (int64_t)pixel_row(a, origin, p, pr, pc) * a.t_pitch + k0;
			float ee[VEC], bb[VEC];
			Vec<VEC>::load(img + off, v);
			if (a.subtract) {
#pragma unroll
				for (int c = 0; c < VEC; c++) v[c] = v[c] - ssub[c];
			}
			Vec<VEC>::load(err + off, ee);
			if (a.bkg_mode == 0) Vec<VEC>::load(bkg + off, bb);
			else {
#pragma unroll
				for (int c = 0; c < VEC; c++) bb[c] = (a.bkg_mode == 1) ? bser[c] : 0.f;
			}
#pragma unroll
			for (int c = 0; c < VEC; c++) e2[c] = ee[c] * ee[c];
			st.side(v, (double)(col0 + pc), (double)(row0 + pr));
			if (has_bkg) st.bkg_terms(bb, y);
		};

		if (M < 8) {
			for (int i = 0; i < M; i++) {
				float v[VEC], e2[VEC], y[VEC];
				fetch(i, v, e2, y);
#pragma unroll
				for (int c = 0; c < VEC; c++) { st.fres[c] += v[c]; st.eres[c] += e2[c]; if (has_bkg) st.bres[c] += y[c]; }
			}
		} else {
			for (int g = 0; g < nblk; g += 8) {
#pragma unroll
				for (int j = 0; j < 8; j++) {
					float v[VEC], e2[VEC], y[VEC];
					fetch(g + j, v, e2, y);
#pragma unroll
					for (int c = 0; c < VEC; c++) {
						if (g == 0) { st.r[c][j] = v[c]; st.e[c][j] = e2[c]; if (has_bkg) st.bk[c][j] = y[c]; }
						else { st.r[c][j] += v[c]; st.e[c][j] += e2[c]; if (has_bkg) st.bk[c][j] += y[c]; }
					}
				}
			}
#pragma unroll
			for (int c = 0; c < VEC; c++) { st.fres[c] = combine8(st.r[c]); st.eres[c] = combine8(st.e[c]); if (has_bkg) st.bres[c] = combine8(st.bk[c]); }
			for (int i = nblk; i < M; i++) {
				float v[VEC], e2[VEC], y[VEC];
				fetch(i, v, e2, y);
#pragma unroll
				for (int c = 0; c < VEC; c++) { st.fres[c] += v[c]; st.eres[c] += e2[c]; if (has_bkg) st.bres[c] += y[c]; }
			}
		}
		// np.sum = 0 + pairwise_sum (identity-initialised reduce)
#pragma unroll
		for (int c = 0; c < VEC; c++) { st.fres[c] = 0.f + st.fres[c]; st.eres[c] = 0.f + st.eres[c]; st.bres[c] = 0.f + st.bres[c]; }
		store_outputs<VEC>(a, target, k0, st, M);
	}
}

// ---- the streamed extraction of the fused per-target kernel ----
//
// The pixel table: what the streamed extraction needs of a mask pixel, built once per target (one lane per pixel) where the stand-
// alone kernels pack the row into the list entry (pack_rows): the byte offset of the pixel's row in the target's cube and its
// 1-based CCD column and row as doubles, exactly the (double)(col0 + pc), (double)(row0 + pr) of extract_small.  Three arrays of
// `entries` elements each (the mask size rounded up to whole groups of 8; the padding repeats the last pixel, so a group's reads
// never clamp), 16-byte aligned: a group's eight entries are two (offsets) and eight (columns, rows) 16-byte reads at an address
// that is the same in every lane, with ONE wait each, and the values arrive as vector operands -- no scalar-register round trip
// and no integer-to-double conversion per pixel and cadence block.
// The offsets are 32-bit: the caller guarantees height * width * t_pitch * 4 < 2^32 (tp_ap::stream_offsets_fit).
struct PixelTable { const double* col; const double* row; const uint32_t* off; };

constexpr int kPixelEntryBytes = 20;
__host__ __device__ inline int pixel_table_entries(int M) { return (M + 7) & ~7; }
__host__ __device__ inline bool stream_offsets_fit(int64_t P, int64_t t_pitch) { return P * t_pitch * 4 < ((int64_t)1 << 32); }

// mem: 16-byte aligned, pixel_table_entries(M) * kPixelEntryBytes bytes, not overlapping list.  list: plain pixel indices.
__device__ __forceinline__ PixelTable build_pixel_table(void* mem, const int* list, int M, const Args& a, int target, int lane, int nlanes)
{
	const int M8 = pixel_table_entries(M);
	double* col = static_cast<double*>(mem);
	double* row = col + M8;
	uint32_t* off = reinterpret_cast<uint32_t*>(row + M8);
	const int col0 = a.stamps[target * 4 + 2] + 1; // 1-based CCD column of stamp column 0
	const int row0 = a.stamps[target * 4 + 0] + 1;
	for (int i = lane; i < M8; i += nlanes) {
		const int p = list[(i < M) ? i : (M - 1)];
		const int pr = p / a.width, pc = p - pr * a.width;
		off[i] = (uint32_t)p * (uint32_t)a.t_pitch * 4u;
		col[i] = (double)(col0 + pc);
		row[i] = (double)(row0 + pr);
	}
	PixelTable t;
	t.col = col; t.row = row; t.off = off;
	return t;
}

// Per-thread state of the streamed extraction for VEC cadences.  The pairwise accumulators start at -0.0: under round-to-nearest
// (-0.0) + x is x for every x (x = -0.0 and +0.0 included, a NaN stays that NaN), so "the first group assigns, later groups add"
// of extract_small is one and the same addition here and no group is special.  NBK = 8 background accumulators per cadence in the
// background-cube mode; ONE in the series mode, where the term does not depend on the pixel: the eight accumulators of extract_small
// all receive the same additions in the same order and hold the same bits, so one chain is kept and read eight times by combine8.
// The leaf's running sum -- combine8 of the full groups, then the tail pixels added in order -- lives in accumulator 0, which is
// free by then; fres / eres / bres only exist at the end of a cadence block.  A mask of fewer than 8 pixels starts that sum at
// -0.0 where extract_small starts at +0.0: the two differ only while every term so far was -0.0, and the closing 0.f + sum of
// np.sum's identity-initialised reduce makes both +0.0.
template <int VEC, int NBK>
struct StreamState {
	float r[VEC][8], e[VEC][8], bk[VEC][NBK];
	float fres[VEC], eres[VEC], bres[VEC];
	double cw[VEC], ccol[VEC], crow[VEC];
	bool f_allnan[VEC], f_allzero[VEC], b_allnan[VEC];

	__device__ __forceinline__ void init() {
#pragma unroll
		for (int c = 0; c < VEC; c++) {
#pragma unroll
			for (int j = 0; j < 8; j++) { r[c][j] = -0.f; e[c][j] = -0.f; }
#pragma unroll
			for (int j = 0; j < NBK; j++) bk[c][j] = -0.f;
			fres[c] = 0.f; eres[c] = 0.f; bres[c] = 0.f;
			cw[c] = 0.0; ccol[c] = 0.0; crow[c] = 0.0;
			f_allnan[c] = true; f_allzero[c] = true; b_allnan[c] = true;
		}
	}
	// CadState::side for one cadence.  The weight is max(x, 0): +0.0 for a NaN and for every value that is not positive (the sign
	// of a zero weight changes none of the three sums: they start at +0.0 and never become -0.0), x otherwise, +inf included.
	// FUSE: col and row are integers below 2^29 in magnitude and w has a 24-bit significand, so col * w and row * w have at most
	// 53 significant bits and are exact in double (no overflow or underflow: float's exponent range plus 29 bits); an exact product
	// makes fma(col, w, acc) = round(acc + col * w) bit for bit the two-operation form.  The caller chooses FUSE per target.
	template <bool FUSE>
	__device__ __forceinline__ void side(int c, float x, double col, double row) {
		f_allnan[c] = f_allnan[c] && (x != x);
		f_allzero[c] = f_allzero[c] && (x == 0.f);
		const double w = (double)__builtin_fmaxf(x, 0.f);
		cw[c] += w;
		if (FUSE) { ccol[c] = __builtin_fma(col, w, ccol[c]); crow[c] = __builtin_fma(row, w, crow[c]); }
		else { ccol[c] += col * w; crow[c] += row * w; }
	}
};

// The extraction of extract_small as a flat software pipeline (the fused per-target kernel, where one wavefront walks all
// cadence blocks of its target): the mask pixels are consumed in groups of 8 from two ping-pong register buffers, the loads
// of group g+1 -- also across cadence blocks -- are in flight while group g is accumulated, and every load is
// unconditional straight-line code (steps past the end repeat the last one) so that only the ping-pong order decides the
// waitcnts.  What a group is (a full group of the pairwise leaf, or the tail that is added in order) is decided once per group;
// the full group's body has no branch.  Pixel order, accumulator assignment and operation order are those of extract_small:
// identical results.
// (an empty statement that holds a wave-uniform value in a scalar register and hides where it came from)
#define TP_AP_KEEP_SCALAR(x) asm volatile("" : "+s"(x))
template <int VEC, bool HAS_SUB, int BKG, bool LDS_SERIES, bool FUSE>
__device__ __forceinline__ void extract_small_stream(const Args& a, int target, const PixelTable& tbl, int M, int q_lane, int q_stride,
	const float* lds_sub = nullptr, const float* lds_ser = nullptr)
{
	// lds_sub / lds_ser: the target's subtracted / background series staged in LDS by the caller (same values as in HBM): a lane's
	// cadences do not change over the pixel groups, so the HBM copy would be re-read once per group (1.85 GB per launch of 10 000
	// targets, measured); LDS reads also stay out of the vector-memory queue that paces the pixel loads
	const int P = a.height * a.width;
	const int64_t tb = (int64_t)target * P * a.t_pitch;
	constexpr bool BKG_CUBE = (BKG == 0), BKG_SERIES = (BKG == 1), HAS_BKG = (BKG != 2);
	// (the three cubes' bases are the same in every lane and stay in scalar registers; a pixel load is scalar base + 32-bit lane offset)
	const char* img = reinterpret_cast<const char*>(a.images + tb);
	const char* err = reinterpret_cast<const char*>(a.images_err + tb);
	const char* bkgc = BKG_CUBE ? reinterpret_cast<const char*>(a.backgrounds + tb) : nullptr;
	const float* bser = BKG_SERIES ? (a.backgrounds + (int64_t)target * a.bkg_series_pitch) : nullptr;
	const float* subp = HAS_SUB ? (a.subtract + (int64_t)target * a.subtract_pitch) : nullptr;
	const int nq = (a.n_cad + VEC - 1) / VEC;
	const int nit = (nq + q_stride - 1) / q_stride;
	StreamState<VEC, BKG_CUBE ? 8 : 1> st;
	st.init();
	if (M == 0) {
		for (int it = 0; it < nit; it++) {
			const int q = q_lane + it * q_stride;
			if (q < nq) store_outputs<VEC>(a, target, q * VEC, st, 0);
		}
		return;
	}
	const int nfull = M >> 3, ntail = M & 7;
	const int spq = nfull + (ntail ? 1 : 0); // pixel groups per cadence block

	struct Buf { float v[8][VEC], e[8][VEC], b[BKG_CUBE ? 8 : 1][VEC], ser[VEC], sub[VEC]; };
	Buf bufA, bufB;
	// (cadence block, group) of the next step to issue and of the next step to consume: the same in every lane
	int it_i = 0, g_i = 0, it_c = 0, g_c = 0;
	auto issue = [&](Buf& B) {
		int q = q_lane + it_i * q_stride;
		q = (q < nq) ? q : (nq - 1);
		const int k0 = q * VEC;
		// (a compile-time choice: a pointer that may be LDS or HBM would turn these into flat loads, which wait for everything.
		// From HBM the series' values travel with the buffer; from LDS consume reads them, with the table's columns and rows)
		if (!LDS_SERIES) {
			if (BKG_SERIES) Vec<VEC>::load(bser + k0, B.ser);
			if (HAS_SUB) Vec<VEC>::load(subp + k0, B.sub);
		}
		const uint4* to = reinterpret_cast<const uint4*>(tbl.off + g_i * 8);
		const uint4 o0 = to[0], o1 = to[1];
		const uint32_t ro[8] = { o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w };
		const uint32_t kb = (uint32_t)k0 * 4u;
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const uint64_t vo = (uint64_t)(ro[j] + kb);
			Vec<VEC>::load(reinterpret_cast<const float*>(img + vo), B.v[j]);
			Vec<VEC>::load(reinterpret_cast<const float*>(err + vo), B.e[j]);
			if (BKG_CUBE) Vec<VEC>::load(reinterpret_cast<const float*>(bkgc + vo), B.b[BKG_CUBE ? j : 0]);
		}
		// the step after this one; past the last step the last one is read again (and never consumed)
		if (++g_i == spq) { g_i = 0; ++it_i; }
		if (it_i == nit) { it_i = nit - 1; g_i = spq - 1; }
	};
	// one pixel of a group: everything except where its flux / err^2 / background terms are added
	auto pixel = [&](const Buf& B, const float (&sub)[VEC], int j, double col, double row, float (&v)[VEC], float (&e2)[VEC], float (&y)[VEC]) {
#pragma unroll
		for (int c = 0; c < VEC; c++) {
			v[c] = HAS_SUB ? (B.v[j][c] - sub[c]) : B.v[j][c];
			e2[c] = B.e[j][c] * B.e[j][c];
			st.template side<FUSE>(c, v[c], col, row);
			if (BKG_CUBE) {
				// np.nansum (photometry.py:201) = np.sum of the values with NaN replaced by 0
				const float b = B.b[BKG_CUBE ? j : 0][c];
				const bool fin = (b == b);
				st.b_allnan[c] = st.b_allnan[c] && !fin;
				y[c] = fin ? b : 0.f;
			}
		}
	};
	auto consume = [&](const Buf& B) {
		if (it_c == nit) return; // (the odd step past the end)
		const int q = q_lane + it_c * q_stride;
		float ser[VEC], sub[VEC], yser[VEC];
#pragma unroll
		for (int c = 0; c < VEC; c++) { ser[c] = B.ser[c]; sub[c] = B.sub[c]; }
		if (LDS_SERIES) {
			const int k0 = ((q < nq) ? q : (nq - 1)) * VEC;
			if (BKG_SERIES) Vec<VEC>::load(lds_ser + k0, ser);
			if (HAS_SUB) Vec<VEC>::load(lds_sub + k0, sub);
		}
		if (BKG_SERIES) {
			// the series' term is the same for every pixel of the cadence block: evaluated once per group
#pragma unroll
			for (int c = 0; c < VEC; c++) { const bool fin = (ser[c] == ser[c]); st.b_allnan[c] = !fin; yser[c] = fin ? ser[c] : 0.f; }
		}
		// the columns and rows of a group's pixels are read NP pixels at a time: all eight would be 32 registers beside the two
		// load buffers, more than three wavefronts per SIMD leave (the buffers of the HBM-series variant and of the background-cube
		// mode are larger still: two pixels at a time there)
		constexpr int NP = (LDS_SERIES && !BKG_CUBE) ? 4 : 2;
		const double2* tc = reinterpret_cast<const double2*>(tbl.col + g_c * 8);
		const double2* tr = reinterpret_cast<const double2*>(tbl.row + g_c * 8);
		if (g_c < nfull) {
#pragma unroll
			for (int h = 0; h < 8 / NP; h++) {
				if (h) __builtin_amdgcn_sched_barrier(0); // (or the scheduler joins the parts' reads again)
				double col[NP], row[NP];
#pragma unroll
				for (int i = 0; i < NP / 2; i++) {
					const double2 cc = tc[h * (NP / 2) + i], rr = tr[h * (NP / 2) + i];
					col[2 * i] = cc.x; col[2 * i + 1] = cc.y; row[2 * i] = rr.x; row[2 * i + 1] = rr.y;
				}
#pragma unroll
				for (int jj = 0; jj < NP; jj++) {
					const int j = NP * h + jj;
					float v[VEC], e2[VEC], y[VEC];
					pixel(B, sub, j, col[jj], row[jj], v, e2, y);
#pragma unroll
					for (int c = 0; c < VEC; c++) { st.r[c][j] += v[c]; st.e[c][j] += e2[c]; if (BKG_CUBE) st.bk[c][BKG_CUBE ? j : 0] += y[c]; }
				}
			}
			if (BKG_SERIES) {
#pragma unroll
				for (int c = 0; c < VEC; c++) st.bk[c][0] += yser[c];
			}
			if (g_c == nfull - 1) {
#pragma unroll
				for (int c = 0; c < VEC; c++) {
					st.r[c][0] = combine8(st.r[c]); st.e[c][0] = combine8(st.e[c]);
					if constexpr (BKG_CUBE) st.bk[c][0] = combine8(st.bk[c]);
					if constexpr (BKG_SERIES) { const float b = st.bk[c][0]; st.bk[c][0] = ((b + b) + (b + b)) + ((b + b) + (b + b)); }
				}
			}
		} else {
			// (the count is taken through a scalar register here: as a loop invariant the seven comparisons would be hoisted as
			// seven lane masks and spilled)
			int cnt = ntail;
			TP_AP_KEEP_SCALAR(cnt);
#pragma unroll
			for (int h = 0; h < 8 / NP; h++) {
				if (NP * h < cnt) {
					double col[NP], row[NP];
#pragma unroll
					for (int i = 0; i < NP / 2; i++) {
						const double2 cc = tc[h * (NP / 2) + i], rr = tr[h * (NP / 2) + i];
						col[2 * i] = cc.x; col[2 * i + 1] = cc.y; row[2 * i] = rr.x; row[2 * i + 1] = rr.y;
					}
#pragma unroll
					for (int jj = 0; jj < NP; jj++) {
						const int j = NP * h + jj;
						if (j < cnt) {
							float v[VEC], e2[VEC], y[VEC];
							pixel(B, sub, j, col[jj], row[jj], v, e2, y);
#pragma unroll
							for (int c = 0; c < VEC; c++) { st.r[c][0] += v[c]; st.e[c][0] += e2[c]; if (HAS_BKG) st.bk[c][0] += BKG_SERIES ? yser[c] : y[c]; }
						}
					}
				}
			}
		}
		if (++g_c == spq) {
			// np.sum = 0 + pairwise_sum (identity-initialised reduce)
#pragma unroll
			for (int c = 0; c < VEC; c++) { st.fres[c] = 0.f + st.r[c][0]; st.eres[c] = 0.f + st.e[c][0]; st.bres[c] = HAS_BKG ? (0.f + st.bk[c][0]) : 0.f; }
			if (q < nq) store_outputs<VEC>(a, target, q * VEC, st, M);
			st.init();
			g_c = 0; ++it_c;
		}
	};
	issue(bufA);
	issue(bufB);
	while (it_c < nit) {
		consume(bufA);
		issue(bufA);
		consume(bufB);
		issue(bufB);
	}
}
#undef TP_AP_KEEP_SCALAR

} // namespace tp_ap

// Launches tp_aperture_big_kernel (masks above kMaxList pixels; it skips all other targets) on ctx's stream.
int tp_aperture_extract_big(tp_ctx* ctx, const tp_ap::Args& a, bool vec4);

// Grow-only device scratch of the context (at least `bytes`), nullptr on failure.
void* tp_ctx_scratch(tp_ctx* ctx, size_t bytes);
