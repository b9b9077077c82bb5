// wcs.hip -- TAN-SIP world coordinate systems (astropy.wcs as ImageMovementKernel('wcs') uses it, image_motion.py:113-421) on
// the device, all in float64.
//
// One frame's WCS is a packed parameter block (TP_WCS_PARAMS doubles, photometry_amd/wcs.py packs it; layout below): the native
// to celestial rotation matrix of CRVAL / LONPOLE, CRPIX, CD and its inverse, the SIP A / B coefficients.  Pixel to world:
// pix2foc (SIP), CD, the TAN deprojection as a native direction-cosine vector (-y, x, 1) / sqrt(1 + x^2 + y^2) and the rotation --
// no trigonometry but for the final (ra, dec).  World to pixel: the transposed rotation, the TAN projection, CD^-1, then
// astropy 4.3's _all_world2pix fixed-point iteration (tolerance, maxiter, detect_divergence, adaptive continuation) for SIP.
//
// The iteration's stopping test is a max over the whole BATCH of points of one call (astropy iterates its vectorised loop while
// nanmax(dn) >= tol^2), so a point's result depends on its batch.  A wave holds one (batch, frame): lanes run over the batch's
// points, any number of them, in two passes.  Pass 1 runs every point alone to its own convergence (first step with dn < tol^2)
// or its first divergence step (dn >= dnprev and dn >= tol^2); a wave max / min gives the batch's last convergence step E and
// first divergence step D, which fix astropy's schedule: the batch loop runs to min(E, maxiter - 1), or switches to the adaptive
// continuation at D when D comes first.  Pass 2 runs every point again under that schedule.  A point whose dn rises back above
// tol^2 after its own convergence (a divergence pass 1 cannot see) is flagged TP_WCS_SCHEDULE: astropy would switch the whole batch
// to the adaptive continuation at that step, so the batch's iteration count and its other points may then differ from astropy's
// (within the tolerance).  A batch of at most 64 points --
// a stamp's catalogue, jitter's one point -- runs astropy's loop itself instead, one point per lane, the batch tests by ballot, in
// one pass (the two forms give the same bits but for that flagged case).  No float atomics, no LDS.
#include "common.h"
#include <cmath>

namespace {

// parameter block layout (doubles)
constexpr int P_ROT = 0;       // [9] native -> celestial rotation, row-major: c = M n
constexpr int P_CRPIX = 9;     // [2] CRPIX1, CRPIX2 (FITS, 1-based)
constexpr int P_CD = 11;       // [4] CD1_1 CD1_2 CD2_1 CD2_2 (degrees / pixel)
constexpr int P_CDINV = 15;    // [4] its inverse
constexpr int P_AORD = 19;     // A_ORDER, B_ORDER (0: no SIP)
constexpr int P_BORD = 20;
constexpr int P_HASSIP = 21;
constexpr int P_A = 24;        // [10][10] A_p_q at p * 10 + q
constexpr int P_B = 124;       // [10][10] B_p_q
static_assert(P_B + 100 == TP_WCS_PARAMS, "parameter block size");

constexpr double kD2R = 3.141592653589793238462643 / 180.0;
constexpr double kR2D = 180.0 / 3.141592653589793238462643;
constexpr int kInf = 0x3fffffff;

struct Pt { double x, y; };

// sum_p u^p sum_q c[p][q] v^q, p + q <= ORD (Horner in both), unrolled so that the wave-uniform coefficient loads issue together.
// ORD is at least the larger of A_ORDER and B_ORDER: the terms above a polynomial's own order are zeros of the packed block, and a
// zero term leaves the Horner sums bit for bit as they are (for finite u, v), so every ORD >= the order gives the same bits.
template <int ORD>
__device__ inline double sip_poly(const double* __restrict__ c, int order, double u, double v) {
	if (ORD == 0) {
		// orders above kMaxUnrolled: the same sums with run-time bounds
		double s = 0.0;
		for (int p = order; p >= 0; p--) {
			double t = 0.0;
			for (int q = order - p; q >= 0; q--) t = t * v + c[p * 10 + q];
			s = s * u + t;
		}
		return s;
	}
	double s = 0.0;
#pragma unroll
	for (int p = ORD; p >= 0; p--) {
		double t = 0.0;
#pragma unroll
		for (int q = ORD - p; q >= 0; q--) t = t * v + c[p * 10 + q];
		s = s * u + t;
	}
	return s;
}

// the SIP order of a frame's block: the larger of A_ORDER and B_ORDER, at least 1
__device__ inline int sip_ord(const double* __restrict__ prm) {
	const int o = (int)fmax(prm[P_AORD], prm[P_BORD]);
	return o < 1 ? 1 : (o > 9 ? 9 : o);
}

// orders 1 .. 5 (TESS FFIs: 4) run unrolled; 6 .. 9 through the run-time loops (ORD 0), which give the same bits
#define WCS_ORD_SWITCH(ord, CALL) switch (ord) { \
	case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; case 5: CALL(5); break; \
	default: CALL(0); break; }

// pix2foc in FITS (1-based) pixel coordinates
template <int ORD>
__device__ inline Pt foc1(const double* __restrict__ prm, double x1, double y1) {
	if (prm[P_HASSIP] == 0.0) return {x1, y1};
	const double u = x1 - prm[P_CRPIX], v = y1 - prm[P_CRPIX + 1];
	const int order = ORD ? ORD : sip_ord(prm);
	return {x1 + sip_poly<ORD>(prm + P_A, order, u, v), y1 + sip_poly<ORD>(prm + P_B, order, u, v)};
}

__device__ inline Pt foc1_any(const double* __restrict__ prm, double x1, double y1) {
	Pt f{x1, y1};
#define WCS_FOC1(O) f = foc1<O>(prm, x1, y1)
	WCS_ORD_SWITCH(sip_ord(prm), WCS_FOC1)
#undef WCS_FOC1
	return f;
}

// focal-plane (1-based) -> celestial unit vector
__device__ inline void foc_to_cos(const double* __restrict__ prm, Pt f, double* c) {
	const double dx = f.x - prm[P_CRPIX], dy = f.y - prm[P_CRPIX + 1];
	const double xi = (prm[P_CD] * dx + prm[P_CD + 1] * dy) * kD2R;
	const double eta = (prm[P_CD + 2] * dx + prm[P_CD + 3] * dy) * kD2R;
	const double s = 1.0 / sqrt(1.0 + xi * xi + eta * eta);
	const double n0 = -eta * s, n1 = xi * s, n2 = s;
	const double* M = prm + P_ROT;
	c[0] = M[0] * n0 + M[1] * n1 + M[2] * n2;
	c[1] = M[3] * n0 + M[4] * n1 + M[5] * n2;
	c[2] = M[6] * n0 + M[7] * n1 + M[8] * n2;
}

// celestial unit vector -> pixel (0-based, before SIP): wcs_world2pix; NaN where the point is on or behind the native equator
__device__ inline Pt cos_to_pix0(const double* __restrict__ prm, double c0, double c1, double c2) {
	const double* M = prm + P_ROT;
	const double n0 = M[0] * c0 + M[3] * c1 + M[6] * c2;
	const double n1 = M[1] * c0 + M[4] * c1 + M[7] * c2;
	const double n2 = M[2] * c0 + M[5] * c1 + M[8] * c2;
	if (!(n2 > 0.0)) return {NAN, NAN};
	const double xi = n1 / n2 * kR2D, eta = -n0 / n2 * kR2D;
	const double u = prm[P_CDINV] * xi + prm[P_CDINV + 1] * eta, v = prm[P_CDINV + 2] * xi + prm[P_CDINV + 3] * eta;
	return {u + prm[P_CRPIX] - 1.0, v + prm[P_CRPIX + 1] - 1.0};
}

// pix2foc(pix, origin 0) - pix0: astropy offsets to 1-based, applies SIP, offsets back
template <int ORD>
__device__ inline Pt dpix_of(const double* __restrict__ prm, Pt pix, Pt pix0) {
	const Pt f = foc1<ORD>(prm, pix.x + 1.0, pix.y + 1.0);
	return {(f.x - 1.0) - pix0.x, (f.y - 1.0) - pix0.y};
}

__device__ inline double sq(Pt d) { return d.x * d.x + d.y * d.y; }

// pass 1: the point alone.  e: first step with dn < tol^2 (or NaN); d: first divergence step (kInf: none)
template <int ORD>
__device__ inline void pass1(const double* __restrict__ prm, Pt pix0, double tol2, int maxiter, int& e, int& d) {
	Pt dp = dpix_of<ORD>(prm, pix0, pix0);
	Pt pix = {pix0.x - dp.x, pix0.y - dp.y};
	double dn = sq(dp);
	d = kInf;
	if (!(dn >= tol2)) { e = 0; return; }
	double dnprev = dn;
	for (int j = 1; j <= maxiter - 1; j++) {
		dp = dpix_of<ORD>(prm, pix, pix0);
		dn = sq(dp);
		if (dn >= dnprev && dn >= tol2) { d = j; e = j + 1; return; }
		pix.x -= dp.x; pix.y -= dp.y;
		dnprev = dn;
		if (!(dn >= tol2)) { e = j; return; }
	}
	e = maxiter;
}

// pass 2: the point under its batch's schedule.  Returns the pixel; status bits; a = adaptive passes run
template <int ORD>
__device__ inline Pt pass2(const double* __restrict__ prm, Pt pix0, bool world_finite, double tol2, int maxiter, int E, int D, int& status, int& a) {
	Pt dp = dpix_of<ORD>(prm, pix0, pix0);
	Pt pix = {pix0.x - dp.x, pix0.y - dp.y};
	double dn = sq(dp), dnprev = dn;
	status = 0;
	a = 0;
	const int jmax = min(E, maxiter - 1);
	const bool switched = D <= jmax;
	const int jend = switched ? D : jmax;
	bool in_ind = false;
	for (int j = 1; j <= jend; j++) {
		dp = dpix_of<ORD>(prm, pix, pix0);
		const double dnj = sq(dp);
		if (switched && j == D) {
			const bool conv = dnj < dnprev;
			if (conv) { pix.x -= dp.x; pix.y -= dp.y; }
			in_ind = dnj >= tol2 && conv;
			if (in_ind) dnprev = dnj;
			dn = dnj;
			break;
		}
		if (dnj >= dnprev && dnj >= tol2) status |= TP_WCS_SCHEDULE;
		pix.x -= dp.x; pix.y -= dp.y;
		dnprev = dnj;
		dn = dnj;
	}
	if (in_ind) {
		for (int k = D + 1; k < maxiter; k++) {
			a++;
			dp = dpix_of<ORD>(prm, pix, pix0);
			const double dnnew = sq(dp);
			dnprev = dn;
			dn = dnnew;
			const bool conv = dnnew < dnprev;
			if (conv) { pix.x -= dp.x; pix.y -= dp.y; }
			if (!(dnnew >= tol2 && conv)) break;
		}
	}
	const bool invalid = !(isfinite(pix.x) && isfinite(pix.y)) && world_finite;
	if ((dn >= tol2 && dn >= dnprev) || invalid) status |= TP_WCS_DIVERGENT;
	if (dn >= tol2 && dn < dnprev && !invalid) status |= TP_WCS_SLOW;
	if (invalid) status |= TP_WCS_INVALID;
	return pix;
}

__device__ inline int wave_max(int v) {
	for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
	return v;
}
__device__ inline int wave_min(int v) {
	for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
	return v;
}

__device__ inline bool cos_finite(const double* c) { return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]); }

// the batch schedule of one frame: (E, D) over the points [lo, hi) (every lane of the wave calls it)
template <int ORD>
__device__ inline void batch_schedule(const double* __restrict__ prm, const double* __restrict__ cosv, int64_t lo, int64_t hi, double tol2,
	int maxiter, int& E, int& D)
{
	int e_max = 0, d_min = kInf;
	for (int64_t i = lo + threadIdx.x; i < hi; i += 64) {
		const double* c = cosv + i * 3;
		int e, d;
		pass1<ORD>(prm, cos_to_pix0(prm, c[0], c[1], c[2]), tol2, maxiter, e, d);
		e_max = max(e_max, e);
		d_min = min(d_min, d);
	}
	E = wave_max(e_max);
	D = wave_min(d_min);
}

// A batch of at most 64 points, one per lane (inactive lanes vote false): astropy's loop itself, the batch-wide tests by ballot,
// in one pass.  k: astropy's iteration count (wave-uniform).
template <int ORD>
__device__ inline Pt wave_batch(const double* __restrict__ prm, Pt pix0, bool world_finite, bool active, double tol2, int maxiter, int& status,
	int& k)
{
	Pt dp = dpix_of<ORD>(prm, pix0, pix0);
	Pt pix = {pix0.x - dp.x, pix0.y - dp.y};
	double dn = sq(dp), dnprev = dn;
	bool switched = false, in_ind = false;
	k = 1;
	while (k < maxiter && __ballot(active && dn >= tol2) != 0) {
		dp = dpix_of<ORD>(prm, pix, pix0);
		const double dnj = sq(dp);
		if (__ballot(active && dnj >= dnprev && dnj >= tol2) != 0) {
			const bool conv = dnj < dnprev;
			if (conv) { pix.x -= dp.x; pix.y -= dp.y; }
			in_ind = active && dnj >= tol2 && conv;
			if (in_ind) dnprev = dnj;
			dn = dnj;
			k++;
			switched = true;
			break;
		}
		pix.x -= dp.x; pix.y -= dp.y;
		dnprev = dnj;
		dn = dnj;
		k++;
	}
	if (switched) {
		while (k < maxiter && __ballot(in_ind) != 0) {
			if (in_ind) {
				dp = dpix_of<ORD>(prm, pix, pix0);
				const double dnnew = sq(dp);
				dnprev = dn;
				dn = dnnew;
				const bool conv = dnnew < dnprev;
				if (conv) { pix.x -= dp.x; pix.y -= dp.y; }
				in_ind = dnnew >= tol2 && conv;
			}
			k++;
		}
	}
	const bool invalid = !(isfinite(pix.x) && isfinite(pix.y)) && world_finite;
	status = 0;
	if ((dn >= tol2 && dn >= dnprev) || invalid) status |= TP_WCS_DIVERGENT;
	if (dn >= tol2 && dn < dnprev && !invalid) status |= TP_WCS_SLOW;
	if (invalid) status |= TP_WCS_INVALID;
	return pix;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------

// pixel -> world of one frame, one point per thread.  mode 0: pix2foc, 1: wcs_pix2world (no SIP), 2: all_pix2world.
__global__ __launch_bounds__(256) void tp_wcs_pix2world_kernel(const double* __restrict__ prm, int64_t n, const double* __restrict__ xy,
	double origin, int mode, double* __restrict__ out, double* __restrict__ cos_out)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const double x1 = xy[2 * i] + (1.0 - origin), y1 = xy[2 * i + 1] + (1.0 - origin);
	const Pt f = mode == 1 ? Pt{x1, y1} : foc1_any(prm, x1, y1);
	if (mode == 0) {
		out[2 * i] = f.x - (1.0 - origin);
		out[2 * i + 1] = f.y - (1.0 - origin);
		return;
	}
	double c[3];
	foc_to_cos(prm, f, c);
	if (out) {
		double ra = atan2(c[1], c[0]) * kR2D;
		if (ra < 0.0) ra += 360.0;
		out[2 * i] = ra;
		out[2 * i + 1] = atan2(c[2], sqrt(c[0] * c[0] + c[1] * c[1])) * kR2D;
	}
	if (cos_out) {
		cos_out[3 * i] = c[0];
		cos_out[3 * i + 1] = c[1];
		cos_out[3 * i + 2] = c[2];
	}
}

__global__ __launch_bounds__(256) void tp_wcs_widen_kernel(int64_t n, const float* __restrict__ in, double* __restrict__ out) {
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[i] = (double)in[i];
}

// (ra, dec) degrees -> celestial unit vectors
__global__ __launch_bounds__(256) void tp_wcs_radec_kernel(int64_t n, const double* __restrict__ radec, double* __restrict__ cosv) {
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const double a = radec[2 * i] * kD2R, d = radec[2 * i + 1] * kD2R;
	const double cd = cos(d);
	cosv[3 * i] = cd * cos(a);
	cosv[3 * i + 1] = cd * sin(a);
	cosv[3 * i + 2] = sin(d);
}

template <int ORD>
__device__ inline void w2p_body(const double* __restrict__ prm, int64_t lo, int64_t hi, const double* __restrict__ cosv, double origin, bool iterate,
	double tol2, int maxiter, double* __restrict__ pout, int32_t* __restrict__ sout, int32_t* __restrict__ iters)
{
	if (iterate && hi - lo <= 64) {
		const int64_t i = lo + threadIdx.x;
		const bool active = i < hi;
		const double* c = cosv + (active ? i : lo) * 3;
		int st, k;
		const Pt p = wave_batch<ORD>(prm, cos_to_pix0(prm, c[0], c[1], c[2]), cos_finite(c), active, tol2, maxiter, st, k);
		if (active) {
			pout[2 * i] = p.x + origin;
			pout[2 * i + 1] = p.y + origin;
			sout[i] = st;
		}
		if (threadIdx.x == 0 && iters) *iters = k;
		return;
	}
	int E = 0, D = kInf;
	if (iterate) batch_schedule<ORD>(prm, cosv, lo, hi, tol2, maxiter, E, D);
	int a_max = 0;
	for (int64_t i = lo + threadIdx.x; i < hi; i += 64) {
		const double* c = cosv + i * 3;
		Pt p = cos_to_pix0(prm, c[0], c[1], c[2]);
		int st = 0, a = 0;
		if (iterate) p = pass2<ORD>(prm, p, cos_finite(c), tol2, maxiter, E, D, st, a);
		a_max = max(a_max, a);
		pout[2 * i] = p.x + origin;
		pout[2 * i + 1] = p.y + origin;
		sout[i] = st;
	}
	a_max = wave_max(a_max);
	if (threadIdx.x == 0 && iters) {
		const int jmax = min(E, maxiter - 1);
		*iters = !iterate ? 0 : (D <= jmax ? D + 1 + a_max : jmax + 1);
	}
}

// world -> pixel: one wave per (batch, frame); grid (n_batches, n_frames).  all = 0: wcs_world2pix.
__global__ __launch_bounds__(64) void tp_wcs_world2pix_kernel(const double* __restrict__ params, int64_t n, const int64_t* __restrict__ offsets,
	const double* __restrict__ cosv, double origin, int all, double tol2, int maxiter, double* __restrict__ pix_out, int32_t* __restrict__ status_out,
	int32_t* __restrict__ iters_out)
{
	const int b = blockIdx.x, f = blockIdx.y;
	const double* prm = params + (int64_t)f * TP_WCS_PARAMS;
	const int64_t lo = offsets[b], hi = min(offsets[b + 1], n);
	double* pout = pix_out + (int64_t)f * n * 2;
	int32_t* sout = status_out + (int64_t)f * n;
	const bool iterate = all && prm[P_HASSIP] != 0.0;
	int32_t* it = iters_out ? iters_out + (int64_t)f * gridDim.x + b : nullptr;
	if (lo >= hi) {
		// an empty batch: nothing to read or write (d_cos may be NULL when n == 0)
		if (threadIdx.x == 0 && it) *it = 0;
		return;
	}
#define WCS_W2P(O) w2p_body<O>(prm, lo, hi, cosv, origin, iterate, tol2, maxiter, pout, sout, it)
	WCS_ORD_SWITCH(sip_ord(prm), WCS_W2P)
#undef WCS_W2P
}

// load_series' test of every frame: the first calc_footprint(axes=(2, 2)) corner, pixel (0, 0), through all_pix2world and back
// through all_world2pix(maxiter, tolerance) as a batch of one; status bits per frame
__global__ __launch_bounds__(256) void tp_wcs_footprint_kernel(const double* __restrict__ params, int n_frames, double tol2, int maxiter,
	int32_t* __restrict__ status_out)
{
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f >= n_frames) return;
	const double* prm = params + (int64_t)f * TP_WCS_PARAMS;
	double c[3];
	foc_to_cos(prm, foc1_any(prm, 1.0, 1.0), c);
	int st = 0;
	if (prm[P_HASSIP] != 0.0) {
		const Pt p0 = cos_to_pix0(prm, c[0], c[1], c[2]);
		int e, d, a;
#define WCS_FOOT(O) pass1<O>(prm, p0, tol2, maxiter, e, d); pass2<O>(prm, p0, cos_finite(c), tol2, maxiter, e, d, st, a)
		WCS_ORD_SWITCH(sip_ord(prm), WCS_FOOT)
#undef WCS_FOOT
	}
	status_out[f] = st;
}

struct PosArgs {
	const double* params;     // [n_frames][TP_WCS_PARAMS]
	int n_frames;
	int64_t n;                // catalogue rows
	const int64_t* offsets;   // [n_batches + 1]
	const double* cosv;       // [n][3] the rows' world directions (reference WCS)
	const float* xy32;        // [n][2] (column, row)
	const float* base_col;    // [n]
	const float* base_row;
	const int64_t* out_index; // [n]: output row, -1 for none
	int64_t n_out;
	int n_cad;
	const int32_t* k1;        // [n_cad]
	const int32_t* k2;        // [n_cad], -1: k1 alone
	const double* dt;         // [n_cad] t2 - t1
	const double* dx;         // [n_cad] t - t1
	double tol2;
	int maxiter;
	double* pos_col;          // [n_out][pitch]
	double* pos_row;
	int64_t pitch;
	int32_t* status;          // [n] OR of the status bits over the cadences (may be null)
};

constexpr int kPosCadTile = 16;

// one cadence of tp_wcs_positions_kernel
template <int ORD>
__device__ inline void pos_cadence(const PosArgs& A, int64_t lo, int64_t hi, int kc, bool ok, bool two, const double* __restrict__ p1,
	const double* __restrict__ p2)
{
	const bool it1 = p1[P_HASSIP] != 0.0, it2 = two && p2[P_HASSIP] != 0.0;
	const double dt = A.dt[kc], dx = A.dx[kc];
	if (hi - lo <= 64) {
		// the whole catalogue in one wave: astropy's loop by ballot, one pass per frame
		const int64_t i = lo + threadIdx.x;
		const bool active = i < hi;
		const int64_t ii = active ? i : lo;
		const double* c = A.cosv + ii * 3;
		const bool wf = cos_finite(c);
		const double x = (double)A.xy32[2 * ii], y = (double)A.xy32[2 * ii + 1];
		int st = 0, s2 = 0, k;
		double jx = NAN, jy = NAN;
		if (ok) {
			Pt q = cos_to_pix0(p1, c[0], c[1], c[2]);
			if (it1) q = wave_batch<ORD>(p1, q, wf, active, A.tol2, A.maxiter, st, k);
			jx = q.x - x;
			jy = q.y - y;
			if (two) {
				Pt r = cos_to_pix0(p2, c[0], c[1], c[2]);
				if (it2) r = wave_batch<ORD>(p2, r, wf, active, A.tol2, A.maxiter, s2, k);
				jx = (r.x - x - jx) / dt * dx + jx;
				jy = (r.y - y - jy) / dt * dx + jy;
			}
		} else {
			st = TP_WCS_INVALID;
		}
		st |= s2;
		if (!active) return;
		const int64_t o = A.out_index[i];
		if (st && A.status) atomicOr(A.status + i, st);
		if (o >= 0 && o < A.n_out) {
			A.pos_col[o * A.pitch + kc] = (double)(float)((double)A.base_col[i] + jx);
			A.pos_row[o * A.pitch + kc] = (double)(float)((double)A.base_row[i] + jy);
		}
		return;
	}
	int E1 = 0, D1 = kInf, E2 = 0, D2 = kInf;
	if (ok && it1) batch_schedule<ORD>(p1, A.cosv, lo, hi, A.tol2, A.maxiter, E1, D1);
	if (it2) batch_schedule<ORD>(p2, A.cosv, lo, hi, A.tol2, A.maxiter, E2, D2);
	for (int64_t i = lo + threadIdx.x; i < hi; i += 64) {
		const int64_t o = A.out_index[i];
		const double* c = A.cosv + i * 3;
		const bool wf = cos_finite(c);
		const double x = (double)A.xy32[2 * i], y = (double)A.xy32[2 * i + 1];
		int st = 0, s2 = 0, a;
		double jx = NAN, jy = NAN;
		if (ok) {
			Pt q = cos_to_pix0(p1, c[0], c[1], c[2]);
			if (it1) q = pass2<ORD>(p1, q, wf, A.tol2, A.maxiter, E1, D1, st, a);
			jx = q.x - x;
			jy = q.y - y;
			if (two) {
				Pt r = cos_to_pix0(p2, c[0], c[1], c[2]);
				if (it2) r = pass2<ORD>(p2, r, wf, A.tol2, A.maxiter, E2, D2, s2, a);
				// scipy's interp1d between the two frames: slope * (t - t1) + y1
				jx = (r.x - x - jx) / dt * dx + jx;
				jy = (r.y - y - jy) / dt * dx + jy;
			}
		} else {
			st = TP_WCS_INVALID;
		}
		st |= s2;
		if (st && A.status) atomicOr(A.status + i, st);
		if (o >= 0 && o < A.n_out) {
			A.pos_col[o * A.pitch + kc] = (double)(float)((double)A.base_col[i] + jx);
			A.pos_row[o * A.pitch + kc] = (double)(float)((double)A.base_row[i] + jy);
		}
	}
}

// LinPSF positions: one wave per (batch, tile of kPosCadTile cadences); grid (n_batches, tiles)
__global__ __launch_bounds__(64) void tp_wcs_positions_kernel(PosArgs A) {
	const int b = blockIdx.x;
	const int64_t lo = A.offsets[b], hi = min(A.offsets[b + 1], A.n);
	if (lo >= hi) return;    // an empty stamp catalogue: no row to read or write
	const int kc0 = blockIdx.y * kPosCadTile, kc1 = min(kc0 + kPosCadTile, A.n_cad);
	for (int kc = kc0; kc < kc1; kc++) {
		const int f1 = A.k1[kc], f2 = A.k2[kc];
		const bool ok = f1 >= 0 && f1 < A.n_frames && f2 < A.n_frames;
		const double* p1 = A.params + (int64_t)(ok ? f1 : 0) * TP_WCS_PARAMS;
		const double* p2 = A.params + (int64_t)(ok && f2 >= 0 ? f2 : 0) * TP_WCS_PARAMS;
		const bool two = ok && f2 >= 0;
		const int ord = max(sip_ord(p1), two ? sip_ord(p2) : 1);
#define WCS_POS(O) pos_cadence<O>(A, lo, hi, kc, ok, two, p1, p2)
		WCS_ORD_SWITCH(ord, WCS_POS)
#undef WCS_POS
	}
}

bool offsets_ok(const int64_t* h, int32_t nb, int64_t n) {
	if (h[0] < 0) return false;
	for (int32_t b = 0; b < nb; b++) if (h[b + 1] < h[b]) return false;
	return h[nb] <= n;
}

} // namespace

extern "C" int tp_wcs_pix2world(tp_ctx* ctx, const double* d_params, int64_t n, const double* d_xy, int32_t origin, int32_t mode, double* d_out,
	double* d_cos)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, n >= 0 && (origin == 0 || origin == 1) && mode >= 0 && mode <= 2, "tp_wcs_pix2world: bad arguments");
	if (n == 0) return TP_OK;
	TP_REQUIRE(ctx, d_params && d_xy && (d_out || (mode != 0 && d_cos)), "tp_wcs_pix2world: null pointer");
	TP_LAUNCH(ctx, TPK_WCS_PIX2WORLD, tp_wcs_pix2world_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_params, n, d_xy, (double)origin,
		(int)mode, d_out, d_cos);
	TP_LAUNCH_CHECK(ctx, "tp_wcs_pix2world_kernel");
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_wcs_radec(tp_ctx* ctx, int64_t n, const double* d_radec, double* d_cos)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, n >= 0, "tp_wcs_radec: bad size");
	if (n == 0) return TP_OK;
	TP_REQUIRE(ctx, d_radec && d_cos, "tp_wcs_radec: null pointer");
	TP_LAUNCH(ctx, TPK_WCS_RADEC, tp_wcs_radec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, n, d_radec, d_cos);
	TP_LAUNCH_CHECK(ctx, "tp_wcs_radec_kernel");
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_wcs_world2pix(tp_ctx* ctx, const double* d_params, int32_t n_frames, int64_t n, int32_t n_batches, const int64_t* h_offsets,
	const double* d_cos, int32_t origin, int32_t all, double tolerance, int32_t maxiter, double* d_pix, int32_t* d_status, int32_t* d_iters)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, n_frames >= 0 && n_frames <= 65535 && n >= 0 && n_batches >= 0 && (origin == 0 || origin == 1) && maxiter >= 0 && tolerance >= 0.0,
		"tp_wcs_world2pix: bad arguments");
	if (n_frames == 0 || n_batches == 0) return TP_OK;
	TP_REQUIRE(ctx, d_params && h_offsets && d_pix && d_status && (n == 0 || d_cos), "tp_wcs_world2pix: null pointer");
	TP_REQUIRE(ctx, offsets_ok(h_offsets, n_batches, n), "tp_wcs_world2pix: batch offsets must rise from >= 0 to <= n");
	int64_t* d_off = nullptr;
	int rc = tp_malloc(ctx, (uint64_t)(n_batches + 1) * sizeof(int64_t), (void**)&d_off);
	if (rc != TP_OK) return rc;
	rc = tp_memcpy_h2d(ctx, d_off, h_offsets, (uint64_t)(n_batches + 1) * sizeof(int64_t));
	if (rc == TP_OK) {
		TP_LAUNCH(ctx, TPK_WCS_WORLD2PIX, tp_wcs_world2pix_kernel, dim3((unsigned)n_batches, (unsigned)n_frames), dim3(64), 0, d_params, n, d_off, d_cos,
			(double)origin, (int)all, tolerance * tolerance, (int)maxiter, d_pix, d_status, d_iters);
		hipError_t e = hipGetLastError();
		if (e != hipSuccess) rc = ctx->fail(TP_ERR_HIP, "tp_wcs_world2pix_kernel", e);
	}
	tp_free(ctx, d_off);
	return rc;
	TP_API_END(ctx)
}

extern "C" int tp_wcs_footprint_check(tp_ctx* ctx, const double* d_params, int32_t n_frames, double tolerance, int32_t maxiter, int32_t* d_status)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, n_frames >= 0 && maxiter >= 0 && tolerance >= 0.0, "tp_wcs_footprint_check: bad arguments");
	if (n_frames == 0) return TP_OK;
	TP_REQUIRE(ctx, d_params && d_status, "tp_wcs_footprint_check: null pointer");
	TP_LAUNCH(ctx, TPK_WCS_FOOTPRINT, tp_wcs_footprint_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, d_params, (int)n_frames,
		tolerance * tolerance, (int)maxiter, d_status);
	TP_LAUNCH_CHECK(ctx, "tp_wcs_footprint_kernel");
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_wcs_star_positions(tp_ctx* ctx, const double* d_params, int32_t n_frames, const double* d_ref_params, int64_t n, int32_t n_batches,
	const int64_t* h_offsets, const float* d_xy32, const float* d_base_col, const float* d_base_row, const int64_t* d_out_index, int64_t n_out,
	int32_t n_cad, const int32_t* d_k1, const int32_t* d_k2, const double* d_dt, const double* d_dx, double tolerance, int32_t maxiter,
	double* d_pos_col, double* d_pos_row, int64_t pos_pitch, int32_t* d_status)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	TP_REQUIRE(ctx, n_frames >= 1 && n >= 0 && n_batches >= 0 && n_out >= 0 && n_cad >= 0 && pos_pitch >= n_cad && maxiter >= 0 && tolerance >= 0.0,
		"tp_wcs_star_positions: bad arguments");
	if (n_batches == 0 || n_cad == 0 || n == 0) return TP_OK;
	TP_REQUIRE(ctx, d_params && d_ref_params && h_offsets && d_xy32 && d_base_col && d_base_row && d_out_index && d_k1 && d_k2 && d_dt && d_dx
		&& (n_out == 0 || (d_pos_col && d_pos_row)), "tp_wcs_star_positions: null pointer");
	TP_REQUIRE(ctx, offsets_ok(h_offsets, n_batches, n), "tp_wcs_star_positions: batch offsets must rise from >= 0 to <= n");
	const unsigned tiles = (unsigned)((n_cad + kPosCadTile - 1) / kPosCadTile);
	TP_REQUIRE(ctx, tiles <= 65535, "tp_wcs_star_positions: too many cadences");
	void *d_off = nullptr, *d_cos = nullptr, *d_xy = nullptr;
	int rc = TP_OK;
	auto alloc = [&](void** p, uint64_t bytes) { if (rc == TP_OK) rc = tp_malloc(ctx, bytes, p); };
	alloc(&d_off, (uint64_t)(n_batches + 1) * sizeof(int64_t));
	alloc(&d_cos, (uint64_t)n * 3 * sizeof(double));
	alloc(&d_xy, (uint64_t)n * 2 * sizeof(double));
	if (rc == TP_OK) rc = tp_memcpy_h2d(ctx, d_off, h_offsets, (uint64_t)(n_batches + 1) * sizeof(int64_t));
	if (rc == TP_OK) {
		// the rows' world directions under the reference WCS (all_pix2world of the float32 catalogue positions)
		TP_LAUNCH(ctx, TPK_WCS_WIDEN, tp_wcs_widen_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, 2 * n, d_xy32, (double*)d_xy);
		TP_LAUNCH(ctx, TPK_WCS_PIX2WORLD, tp_wcs_pix2world_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_ref_params, n,
			(const double*)d_xy, 0.0, 2, (double*)nullptr, (double*)d_cos);
		PosArgs A{d_params, (int)n_frames, n, (const int64_t*)d_off, (const double*)d_cos, d_xy32, d_base_col, d_base_row, d_out_index, n_out,
			(int)n_cad, d_k1, d_k2, d_dt, d_dx, tolerance * tolerance, (int)maxiter, d_pos_col, d_pos_row, pos_pitch, d_status};
		TP_LAUNCH(ctx, TPK_WCS_POSITIONS, tp_wcs_positions_kernel, dim3((unsigned)n_batches, tiles), dim3(64), 0, A);
		hipError_t e = hipGetLastError();
		if (e != hipSuccess) rc = ctx->fail(TP_ERR_HIP, "tp_wcs_positions_kernel", e);
	}
	for (void* p : {d_off, d_cos, d_xy}) if (p) tp_free(ctx, p);
	return rc;
	TP_API_END(ctx)
}
