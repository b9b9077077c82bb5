// linpsf_plan_rules.h -- what the LinPSF plan decides (linpsf_plan.hip: tp_linpsf_plan_kernel), each rule stated once over plain
// values: which kernel fits a target, how the matrix-core fit walks its pixels and cadences, where its coefficients lie.  No device
// code, no HIP runtime: the plan kernel calls these from its parallel plumbing, tests/hostsim/linpsf_plan_host.cpp composes them
// serially under AddressSanitizer and UBSan, and tests/test_linpsf_plan_host.py holds that to linpsf_common.plan_class.
// (The build sets -ffp-contract=off: an expression gives the same bits here as written out in a kernel.)  The table origins
// (valid, ax0, by0) of a position come from axis_phase (linpsf_dev.h); the rules take them as inputs.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TP_RULE __host__ __device__
#else
#define TP_RULE
#endif

namespace tp_linpsf {

constexpr int kMaxStars = 8;      // register-resident vector-ALU kernels (fit2 / direct)
constexpr int kMfmaStars = 4;     // matrix-core kernel (linpsf_mfma.hip)
constexpr int kMfmaPixels = 256;  // pixels of a target's union list U (16 tiles of 16)
constexpr int kMaxOrigins = 36;   // a star that visits more table origins sends its target to the direct kernel

// plan of one fitted star: the table origins its cadences visit and the pixels its cut-off circle can reach
struct StarPlan { int axmin, bymin, nby, nc, jmin, jmax, imin, imax; long long item_off; };

// matrix-core path, per target: the pixels inside the cut-off of ANY fitted star at ANY cadence form the list U (ordered by
// which stars reach them -- Gray-code order of the membership bits, then raster -- so that the pixels of one star are
// contiguous), cut into tiles of 16; star s touches the tiles of `tiles[s]`.
struct MPlan {
	int32_t n_pix, n_tiles;
	uint32_t tiles[kMfmaStars];
	uint32_t edge_tiles[kMfmaStars];   // tiles with a pixel that is inside the star's cut-off at some cadences only
	int32_t n_seg;                     // segments of the series (records target * kMfmaSegs .. + n_seg of the segment array)
};
// The series of a target is cut into SEGMENTS of consecutive 16-cadence tiles inside which every fitted star visits at most
// kMfmaSpan knot intervals per axis: a star that drifts across the pixel during the series (pointing drift, velocity aberration:
// half a pixel is 4.5 knot intervals) stays on the matrix cores, each stretch of the series with the spline of the intervals it
// visits THEN.  Without drift the jitter gives one segment.
// Per (target, segment): the coefficients of ONE tensor-product quartic spline per star over its na x nb intervals
// (linpsf_mfma.hip), laid out as the A operands of the matrix instruction: [star][rank of the tile among its tiles][step][64
// lanes] doubles, the whole segment contiguous from `koff` (that image is copied to LDS as it is), star s from
// `koff + 64 * ksub[s]`, `mfma_steps(na, nb)` steps per tile.  One workgroup of the fit kernel per segment.
struct SegPlan {
	int32_t target;
	int32_t tile0, tile1;              // 16-cadence tiles [tile0, tile1) of the series
	int32_t kdoubles;                  // size of the segment's image (a multiple of 64)
	int64_t koff;                      // doubles from the start of the matrix-core store
	int32_t axmin[kMfmaStars], bymin[kMfmaStars];   // first knot interval the star visits in this segment, per axis
	uint16_t ksub[kMfmaStars];         // in blocks of 64 doubles
	uint8_t na[kMfmaStars], nb[kMfmaStars];   // knot intervals visited along x / y (1..3; 0: the star is never on the stamp)
};
constexpr int kMfmaSpan = 3;          // knot intervals per axis a star may visit inside a segment
constexpr int kMfmaSegs = 8;          // segments per target (more: the vector-ALU kernels take the target)
constexpr int kMfmaCadTiles = 256;    // 16-cadence tiles of a series the plan kernel can cut into segments (4096 cadences: a sector at 600 s)
// steps of v_mfma_f64_16x16x4_f64 per (star, pixel tile): (4 + na) basis functions of x times the first four of y, then two steps
// for each of the nb remaining basis functions of y -- except for the commonest case, 2 x 2 intervals (36 products), which is
// packed into 9 steps instead of 10: the half-empty second step of y basis function 4 also carries x basis functions 0, 1 of y
// basis function 5, and one more step the other four (mfma_is22)
TP_RULE constexpr bool mfma_is22(int na, int nb) { return na == 2 && nb == 2; }
TP_RULE constexpr int mfma_steps(int na, int nb) { return mfma_is22(na, nb) ? 9 : ((4 + na) + 2 * nb); }
// LDS bytes for the coefficient image of a segment: "small" leaves room for two workgroups per CU, "large" (three and four
// stars only: their kernels run one workgroup per CU anyway) takes the LDS of the CU
constexpr int kMfmaLdsSmall = 75776, kMfmaLdsLarge = 157696;
// the plan kernel lists the targets and the segments of the matrix-core path by their number of fitted stars: class = stars - 1
constexpr int kMfmaClasses = kMfmaStars;
// counters the plan kernel keeps (64-bit words of one 256-byte block): kTotClass0 + c targets, kTotSeg0 + c segments of class c
enum { kTotPolyItems = 0, kTotKDoubles = 1, kTotPolyTargets = 2, kTotDirectTargets = 3, kTotGeneral = 4, kTotClass0 = 8, kTotSeg0 = 16, kTotCount = 24 };

// `todo` flag of a target (written by the plan kernel): which kernel fits it
enum { kPathPoly = 0, kPathDirect = 1, kPathMfma = 2 };

//--------------------------------------------------------------------------------------------------
// the box of a star over its series
//--------------------------------------------------------------------------------------------------
// table origins visited and pixels the cut-off circle can reach, over all valid cadences (max < min: none yet)
struct StarBox { int axmin, axmax, bymin, bymax, jmin, jmax, imin, imax; };
constexpr int kBoxNone = 0x7fffffff;

TP_RULE inline void box_clear(StarBox& b)
{
	b.axmin = b.bymin = b.jmin = b.imin = kBoxNone;
	b.axmax = b.bymax = b.jmax = b.imax = -kBoxNone;
}

// what one valid cadence adds: lowest / highest of {origin along x, origin along y, column, row} -- the order of StarBox's pairs
TP_RULE inline void cadence_box(int ax0, int by0, double srow, double scol, double cutoff, int (&v0)[4], int (&v1)[4])
{
	v0[0] = ax0; v0[1] = by0; v0[2] = (int)floor(scol - cutoff); v0[3] = (int)floor(srow - cutoff);
	v1[0] = ax0; v1[1] = by0; v1[2] = (int)ceil(scol + cutoff); v1[3] = (int)ceil(srow + cutoff);
}

// the box clamped to the stamp as the star's plan (item_off 0); nc == 0: never a valid position (an all-zero column) or never on the stamp
TP_RULE inline void star_plan_of(StarBox b, int height, int width, StarPlan& q)
{
	q.axmin = q.bymin = 0; q.nby = 1; q.nc = 0; q.jmin = q.imin = 0; q.jmax = q.imax = -1; q.item_off = 0;
	if (b.axmax < b.axmin) return;
	if (b.jmin < 0) b.jmin = 0;
	if (b.jmax > width - 1) b.jmax = width - 1;
	if (b.imin < 0) b.imin = 0;
	if (b.imax > height - 1) b.imax = height - 1;
	if (b.jmax < b.jmin || b.imax < b.imin) return;
	q.axmin = b.axmin; q.bymin = b.bymin; q.nby = b.bymax - b.bymin + 1; q.nc = (b.axmax - b.axmin + 1) * q.nby;
	q.jmin = b.jmin; q.jmax = b.jmax; q.imin = b.imin; q.imax = b.imax;
}

// Which vector-ALU kernel takes a target the matrix cores do not: the polynomial fit, or -- a star visits more origins than
// kMaxOrigins: pointing excursions over many knots -- the general direct kernel.
TP_RULE inline int fallback_path(const StarPlan* spl, int ns)
{
	bool too_many = false;
	for (int s = 0; s < ns; ++s) if (spl[s].nc > kMaxOrigins) too_many = true;
	return too_many ? kPathDirect : kPathPoly;
}

// item = (pixel of the star's box, origin), 25 doubles each in the polynomial store: every star's first item counted from the
// target's first; returns the target's items
TP_RULE inline long long poly_item_offsets(StarPlan* spl, int ns)
{
	long long items = 0;
	for (int s = 0; s < ns; ++s) {
		StarPlan& q = spl[s];
		q.item_off = items;
		if (q.nc > 0) items += (long long)q.nc * (q.jmax - q.jmin + 1) * (q.imax - q.imin + 1);
	}
	return items;
}

//--------------------------------------------------------------------------------------------------
// segments of the series (matrix-core path)
//--------------------------------------------------------------------------------------------------
// A target without a fitted star -- its own catalogue entry dropped for a NaN magnitude or position -- has no class list: the
// polynomial path finalises it as 'All target flux values are NaN'.
TP_RULE inline bool want_segments(int use_mfma, int ns) { return use_mfma && ns >= 1 && ns <= kMfmaStars; }
// ... and the pixel numbers of the union list are 16-bit, the plan kernel holds kMfmaCadTiles tile records
TP_RULE inline bool segments_possible(bool want, int height, int width, int n_cad) { return want && height * width <= 65535 && n_cad <= 16 * kMfmaCadTiles; }

// the span test: the knot intervals lo .. hi a star visits along an axis stay within kMfmaSpan (hi < lo: it visits none)
TP_RULE inline bool span_fits(int lo, int hi) { return !(hi >= lo && hi - lo + 1 > kMfmaSpan); }

// what the walk keeps of an interval index per tile of cadences: 16 bits (an index beyond them -- a position thousands of pixels off --
// can only come with others that are not: the span test then refuses the target; clamping keeps the order)
TP_RULE inline short tile_record(int v) { return (short)((v < -32767) ? -32767 : ((v > 32766) ? 32766 : v)); }

constexpr int kTileNone = 32767, kTileNoneHigh = -32768;   // lowest / highest interval of a tile or an open segment without a valid position
TP_RULE inline void ranges_clear(int (&lo)[kMfmaStars][2], int (&hi)[kMfmaStars][2])
{
	for (int s = 0; s < kMfmaStars; ++s) { lo[s][0] = lo[s][1] = kTileNone; hi[s][0] = hi[s][1] = kTileNoneHigh; }
}

// The whole series as one segment -- no star leaves its three intervals (no drift) -- with the ranges of the stars' boxes; false
// where a star goes beyond the span, or beyond what the 16-bit tile records of the walk hold
TP_RULE inline bool whole_series_ranges(const StarBox* sbox, int ns, int (&lo)[kMfmaStars][2], int (&hi)[kMfmaStars][2])
{
	ranges_clear(lo, hi);
	bool whole = true;
	for (int s = 0; s < ns; ++s) {
		const StarBox b = sbox[s];
		if (b.axmax < b.axmin) continue;
		if (!span_fits(b.axmin, b.axmax) || !span_fits(b.bymin, b.bymax) || b.axmin < -32000 || b.axmax > 32000 || b.bymin < -32000 || b.bymax > 32000) whole = false;
		lo[s][0] = b.axmin; hi[s][0] = b.axmax; lo[s][1] = b.bymin; hi[s][1] = b.bymax;
	}
	return whole;
}

// one segment of a target's series: the knot intervals every star visits in it (lo / hi per star and axis; hi < lo: never valid)
TP_RULE inline void emit_segment(SegPlan& g, int target, int t0, int t1, const int (&lo)[kMfmaStars][2], const int (&hi)[kMfmaStars][2],
	int ns, const StarPlan* spl)
{
	g.target = target; g.tile0 = t0; g.tile1 = t1; g.kdoubles = 0; g.koff = 0;
	for (int s = 0; s < kMfmaStars; ++s) {
		const bool any = (s < ns) && (hi[s][0] >= lo[s][0]) && (hi[s][1] >= lo[s][1]) && (spl[s].nc > 0);
		g.axmin[s] = any ? lo[s][0] : 0; g.bymin[s] = any ? lo[s][1] : 0;
		g.na[s] = (uint8_t)(any ? (hi[s][0] - lo[s][0] + 1) : 0); g.nb[s] = (uint8_t)(any ? (hi[s][1] - lo[s][1] + 1) : 0);
		g.ksub[s] = 0;
	}
}

//--------------------------------------------------------------------------------------------------
// the union list of pixels (matrix-core path)
//--------------------------------------------------------------------------------------------------
// squared radii: a pixel nearer than `reach` to the rectangle a star's position sweeps is in the list; one whose farthest corner of
// that rectangle is not nearer than `always` is inside the cut-off at some positions of the star and outside at others: an "edge" pixel
TP_RULE inline double pixel_reach2(double cutoff) { return (cutoff + 1e-6) * (cutoff + 1e-6); }
TP_RULE inline double pixel_always2(double cutoff) { return (cutoff - 1e-6) * (cutoff - 1e-6); }

// pixel (i, j) against the rectangle {row min, row max, column min, column max} of a star's valid positions: 0 out of reach, 1 inside
// at every position, 3 an edge pixel
TP_RULE inline unsigned pixel_membership(int i, int j, const double (&range)[4], double reach, double always)
{
	const double dr = fmax(0.0, fmax(range[0] - (double)i, (double)i - range[1]));
	const double dc = fmax(0.0, fmax(range[2] - (double)j, (double)j - range[3]));
	if (!(dr * dr + dc * dc < reach)) return 0u;
	const double fr = fmax(fabs((double)i - range[0]), fabs((double)i - range[1]));
	const double fc = fmax(fabs((double)j - range[2]), fabs((double)j - range[3]));
	return (fr * fr + fc * fc < always) ? 1u : 3u;
}

// inverse of the reflected Gray code n ^ (n >> 1) on 4 bits: the place of a membership pattern in the order 1,3,2,6,7,5,4,12,...
TP_RULE inline unsigned gray_rank4(unsigned g) { g ^= g >> 2; g ^= g >> 1; return g & 15u; }

// the key the list is ordered by: membership pattern (Gray rank), interior pixels before edge pixels, raster; `sig` / `edge`: bit s
// for star s, p < 65536 the pixel
TP_RULE inline unsigned pixel_key(unsigned sig, unsigned edge, int p)
{
	return (gray_rank4(sig) << 25) | ((edge ? 1u : 0u) << 24) | (edge << 20) | (sig << 16) | (unsigned)p;
}
TP_RULE inline uint16_t key_pixel(unsigned key) { return (uint16_t)(key & 0xffffu); }   // the entry of ulist
TP_RULE inline unsigned key_sig(unsigned key) { return (key >> 16) & 15u; }
TP_RULE inline unsigned key_edge(unsigned key) { return (key >> 20) & 15u; }
TP_RULE inline uint8_t key_usig(unsigned key) { return (uint8_t)(key_sig(key) | (key_edge(key) << 4)); }   // the entry of usig

//--------------------------------------------------------------------------------------------------
// the coefficient images of a target's segments (matrix-core path)
//--------------------------------------------------------------------------------------------------
TP_RULE inline void make_mplan(MPlan& mp, int n_pix, int nseg, int ns, const unsigned* tiles, const unsigned* edge_tiles)
{
	mp.n_pix = n_pix; mp.n_tiles = (n_pix + 15) >> 4; mp.n_seg = nseg;
	for (int s = 0; s < kMfmaStars; ++s) {
		mp.tiles[s] = (s < ns) ? tiles[s] : 0u;
		mp.edge_tiles[s] = (s < ns) ? edge_tiles[s] : 0u;
	}
}

// Per segment one spline per star over the knot intervals it visits there (at most 3 x 3): ksub, kdoubles and koff (counted from the
// target's first image) of every segment, `total` doubles in all.  False where a segment's image goes beyond the LDS of its class:
// the vector-ALU kernels take the target.
TP_RULE inline bool size_segments(SegPlan* seg, int nseg, int ns, const MPlan& mp, long long& total)
{
	bool fits = true;
	total = 0;
	for (int i = 0; i < nseg; ++i) {
		SegPlan& g = seg[i];
		long long blocks = 0;
		for (int s = 0; s < kMfmaStars; ++s) {
			g.ksub[s] = (uint16_t)blocks;
			if (g.na[s] > 0) blocks += (long long)__builtin_popcount(mp.tiles[s]) * mfma_steps(g.na[s], g.nb[s]);
		}
		if (blocks * 512 > ((ns <= 1) ? kMfmaLdsSmall : kMfmaLdsLarge)) fits = false;
		g.kdoubles = (int32_t)(blocks * 64);
		g.koff = total;
		total += blocks * 64;
	}
	return fits;
}

//--------------------------------------------------------------------------------------------------
// the order of the cadences (polynomial fit): sorted by the origins of all stars, the cadence in the low 13 bits
//--------------------------------------------------------------------------------------------------
// the key so far with star q's origin at the cadence appended (`valid`: both axes gave an origin)
TP_RULE inline unsigned long long cadence_key_star(unsigned long long key, const StarPlan& q, bool valid, int ax0, int by0)
{
	const int cc = (valid && q.nc > 0) ? ((ax0 - q.axmin) * q.nby + (by0 - q.bymin)) : 0;
	return key * (unsigned long long)(kMaxOrigins + 1) + (unsigned long long)cc;
}
TP_RULE inline unsigned long long cadence_key_close(unsigned long long key, int k) { return key * 8192ull + (unsigned long long)k; }
TP_RULE inline int key_cadence(unsigned long long key) { return (int)(key & 8191ull); }

} // namespace tp_linpsf
