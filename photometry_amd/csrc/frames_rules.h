// frames_rules.h -- everything of the frames engine (frames.cpp) that needs no device: the catalogue index and the per-stamp selection
// (pipeline._CatalogIndex, _catalogs_of_stamps), the layouts of the packed output block (comm.packed_block_layout) and of the metadata
// block (pipeline.ApertureBatch), the round planner, the plugin's per-target decision (stamps.py, plugins.mask_outcome), numpy's
// pairwise sum and the size classes of the page-locked pool.  Host code only, no HIP: tests/hostsim/frames_rules_host.cpp compiles it
// under AddressSanitizer and UBSan, and tests/test_frames_rules_host.py holds it to the Python it restates, bit for bit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace frames_rules {

constexpr int kResizeStep = 10;          // photometry.py:124-131
constexpr int kEdgeBits = 2 | 4 | 8 | 16;
constexpr int32_t kStatusError = 2;      // TP_STATUS_ERROR (include/tessphot_hip.h)

inline int64_t round_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }

// size class of a page-locked block: powers of two from 64 KiB to 1 MiB, above that eighths of the power of two below
inline size_t size_class(size_t n) {
	size_t p = 65536;
	while (p < n && p < ((size_t)1 << 20)) p *= 2;
	if (n <= p) return p;
	p = (size_t)1 << 20;
	while (p * 2 <= n) p *= 2;
	const size_t step = p / 8;
	return (n + step - 1) / step * step;
}

// numpy's pairwise summation of a contiguous float64 vector (np.add.reduce): what np.nansum does after replacing the NaNs
inline double np_pairwise_sum(const double* a, int64_t n) {
	if (n < 8) { double r = 0.0; for (int64_t i = 0; i < n; ++i) r += a[i]; return r; }
	if (n <= 128) {
		double r[8];
		for (int j = 0; j < 8; ++j) r[j] = a[j];
		int64_t i = 8;
		for (; i < n - (n % 8); i += 8) for (int j = 0; j < 8; ++j) r[j] += a[i + j];
		double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
		for (; i < n; ++i) res += a[i];
		return res;
	}
	int64_t n2 = n / 2;
	n2 -= n2 % 8;
	return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// ---- the catalogue of a region, binned into cells of 16 x 16 pixels (stars sorted by cell) ------------------------------------
struct CatalogIndex {
	int64_t n = 0;
	std::vector<int64_t> starid;
	std::vector<float> tmag;
	std::vector<double> row, col;
	int64_t cell = 16, r0 = 0, c0 = 0, n_cr = 1, n_cc = 1;
	std::vector<int64_t> order, cell_start;

	// pipeline._CatalogIndex: cells of 16 x 16 pixels from the floor of the smallest row / column; stars without a position go
	// to a cell no stamp asks for
	void build(int64_t n_stars, const int64_t* h_starid, const float* h_tmag, const double* h_row, const double* h_column) {
		n = n_stars;
		starid.assign(h_starid, h_starid + n_stars);
		tmag.assign(h_tmag, h_tmag + n_stars);
		row.assign(h_row, h_row + n_stars);
		col.assign(h_column, h_column + n_stars);
		double rmin = INFINITY, cmin = INFINITY;
		for (int64_t i = 0; i < n_stars; ++i) {
			if (std::isfinite(row[i])) rmin = std::min(rmin, row[i]);
			if (std::isfinite(col[i])) cmin = std::min(cmin, col[i]);
		}
		r0 = std::isfinite(rmin) ? (int64_t)std::floor(rmin) : 0;
		c0 = std::isfinite(cmin) ? (int64_t)std::floor(cmin) : 0;
		std::vector<int64_t> cr(n_stars, 0), cc(n_stars, 0);
		int64_t crmax = 0, ccmax = 0;
		for (int64_t i = 0; i < n_stars; ++i) {
			if (std::isfinite(row[i]) && std::isfinite(col[i])) {
				cr[i] = (int64_t)std::floor((row[i] - (double)r0) / (double)cell);
				cc[i] = (int64_t)std::floor((col[i] - (double)c0) / (double)cell);
				crmax = std::max(crmax, cr[i]); ccmax = std::max(ccmax, cc[i]);
			}
		}
		n_cr = crmax + 1; n_cc = ccmax + 1;
		const int64_t n_cells = n_cr * n_cc;
		std::vector<int64_t> cid(n_stars);
		for (int64_t i = 0; i < n_stars; ++i)
			cid[i] = (std::isfinite(row[i]) && std::isfinite(col[i]) && cr[i] >= 0 && cc[i] >= 0) ? cr[i] * n_cc + cc[i] : n_cells;
		order.resize(n_stars);
		for (int64_t i = 0; i < n_stars; ++i) order[i] = i;
		std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return cid[a] < cid[b]; });
		cell_start.assign(n_cells + 2, 0);
		for (int64_t i = 0; i < n_stars; ++i) cell_start[cid[i] + 1] += 1;
		for (int64_t k = 0; k <= n_cells; ++k) cell_start[k + 1] += cell_start[k];
	}
};

// the catalogue stars of a run of stamps in CSR form: what pipeline._catalogs_of_stamps returns
struct Selection {
	std::vector<int64_t> cat_offsets{0}, starid;
	std::vector<float> tmag, row, col, row_stamp, col_stamp;
	int64_t n_cat() const { return (int64_t)starid.size(); }
	// the stamps of `o` behind this one's
	void append(const Selection& o) {
		const int64_t base = n_cat();
		for (size_t j = 1; j < o.cat_offsets.size(); ++j) cat_offsets.push_back(base + o.cat_offsets[j]);
		starid.insert(starid.end(), o.starid.begin(), o.starid.end());
		tmag.insert(tmag.end(), o.tmag.begin(), o.tmag.end());
		row.insert(row.end(), o.row.begin(), o.row.end());
		col.insert(col.end(), o.col.begin(), o.col.end());
		row_stamp.insert(row_stamp.end(), o.row_stamp.begin(), o.row_stamp.end());
		col_stamp.insert(col_stamp.end(), o.col_stamp.begin(), o.col_stamp.end());
	}
};

// the stars inside every stamp plus its 5-pixel buffer, in catalogue order, with the float32 stamp coordinates of
// BasePhotometry.catalog (BasePhotometry.py:1094-1181) -- pipeline._catalogs_of_stamps, stamp by stamp.  `stamps` is [..][4]; the
// stamps selected are those at idx[0 .. n_idx)
inline Selection select_catalog(const CatalogIndex& c, const int64_t* stamps, const int32_t* idx, size_t n_idx)
{
	Selection out;
	const double buffer = 5.0;
	const int64_t B = c.cell;
	std::vector<int64_t> found;
	auto clipi = [](int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); };
	for (size_t k = 0; k < n_idx; ++k) {
		const int64_t* st = &stamps[(size_t)idx[k] * 4];
		const double rlo = (double)st[0] - 0.5 - buffer, rhi = (double)st[1] - 0.5 + buffer;
		const double clo = (double)st[2] - 0.5 - buffer, chi = (double)st[3] - 0.5 + buffer;
		found.clear();
		if (c.n > 0) {
			const int64_t cr0 = clipi((int64_t)std::floor((rlo - (double)c.r0) / (double)B), 0, c.n_cr - 1);
			const int64_t cr1 = clipi((int64_t)std::floor((rhi - (double)c.r0) / (double)B), -1, c.n_cr - 1);
			const int64_t cc0 = clipi((int64_t)std::floor((clo - (double)c.c0) / (double)B), 0, c.n_cc - 1);
			const int64_t cc1 = clipi((int64_t)std::floor((chi - (double)c.c0) / (double)B), -1, c.n_cc - 1);
			if (cc1 >= cc0)
				for (int64_t cr = cr0; cr <= cr1; ++cr) {
					const int64_t a = c.cell_start[cr * c.n_cc + cc0], b = c.cell_start[cr * c.n_cc + cc1 + 1];
					for (int64_t p = a; p < b; ++p) {
						const int64_t s = c.order[p];
						if (c.row[s] >= rlo && c.row[s] < rhi && c.col[s] >= clo && c.col[s] < chi) found.push_back(s);
					}
				}
			std::sort(found.begin(), found.end());
		}
		for (int64_t s : found) {
			out.starid.push_back(c.starid[s]);
			out.tmag.push_back(c.tmag[s]);
			out.col.push_back((float)c.col[s]);
			out.row.push_back((float)c.row[s]);
			out.col_stamp.push_back((float)(c.col[s] - (double)st[2]));
			out.row_stamp.push_back((float)(c.row[s] - (double)st[0]));
		}
		out.cat_offsets.push_back(out.n_cat());
	}
	return out;
}

// ---- the packed output block of a group: comm.packed_block_layout(m, T, H, W, n_cat = cat_capacity, extras = True) -------------
struct BlockLayout {
	enum Field { LC, CONTAMINATION, STATUS, FLAGS, MASK, CAT_IN_MASK, SUMIMAGE, DIAGNOSTICS, N_FIELDS };
	uint64_t off[N_FIELDS] = {};
	uint64_t nbytes = 0;
	BlockLayout() {}
	BlockLayout(int64_t m, int64_t T, int64_t H, int64_t W, int64_t cat_capacity) {
		const uint64_t P = (uint64_t)H * W;
		const uint64_t size[N_FIELDS] = {(uint64_t)5 * m * T * 8, (uint64_t)m * 8, (uint64_t)m * 4, (uint64_t)m * 4, (uint64_t)m * P,
			(uint64_t)cat_capacity, (uint64_t)m * P * 8, (uint64_t)m * 10 * 8};
		for (int f = 0; f < N_FIELDS; ++f) { off[f] = nbytes; nbytes = (uint64_t)round_up((int64_t)(nbytes + size[f]), 256); }
	}
	template <class T> T* at(void* base, Field f) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off[f]); }
	template <class T> const T* at(const void* base, Field f) const { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off[f]); }
};

// ---- the metadata of a group as ONE block (the `fields` of pipeline.ApertureBatch): every field at a multiple of 256 bytes and at
// least 16 bytes long
struct MetaLayout {
	enum Field { QUALITY, TIME, STAMPS, CAT_OFFSETS, CAT_STARID, CAT_TMAG, CAT_ROW, CAT_COLUMN, CAT_ROW_STAMP, CAT_COLUMN_STAMP,
		TARGET_ROW, TARGET_COLUMN, TARGET_TMAG, TARGET_STARID, N_FIELDS };
	size_t off[N_FIELDS] = {}, size[N_FIELDS] = {};
	size_t nbytes = 0;
	MetaLayout() {}
	MetaLayout(int64_t T, int64_t m, int64_t n_cat) {
		const size_t t = (size_t)T, n = (size_t)m, nc = (size_t)n_cat;
		const size_t s[N_FIELDS] = {t * 4, t * 8, n * 16, (n + 1) * 8, nc * 8, nc * 4, nc * 4, nc * 4, nc * 4, nc * 4, n * 8, n * 8, n * 8, n * 8};
		for (int f = 0; f < N_FIELDS; ++f) {
			size[f] = s[f];
			off[f] = nbytes;
			nbytes = (size_t)round_up((int64_t)(nbytes + std::max(s[f], (size_t)16)), 256);
		}
	}
	template <class T> T* at(void* base, Field f) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off[f]); }
};

// ---- the groups of a round (targets that share a stamp size, by size key h * 100000 + w, ascending), cut into pieces of at most
// `budget` bytes of device memory; the pieces that run side by side (a part) stay under the budget together -----------------------
struct Piece { std::vector<int32_t> idx; int32_t H, W; double nbytes; };

inline std::vector<std::vector<Piece>> plan_round(const std::vector<int32_t>& active, const int64_t* stamps, int32_t T, bool cubes_needed, double budget)
{
	const int64_t pitch = round_up(T, 32);
	std::map<int64_t, std::vector<int32_t>> by_size;
	for (int32_t i : active) {
		const int64_t h = stamps[(size_t)i * 4 + 1] - stamps[(size_t)i * 4], w = stamps[(size_t)i * 4 + 3] - stamps[(size_t)i * 4 + 2];
		by_size[h * 100000 + w].push_back(i);
	}
	std::vector<std::vector<Piece>> parts(1);
	double acc = 0.0;
	for (auto& kv : by_size) {
		const int32_t H = (int32_t)(kv.first / 100000), W = (int32_t)(kv.first % 100000);
		const double per_target = (cubes_needed ? 3.0 * H * W * (double)pitch * 4 : 0.0) + 5.0 * T * 8 + (double)H * W * 13 + 256;
		const int64_t nmax = std::max<int64_t>(1, (int64_t)std::floor(budget / per_target));
		for (size_t a0 = 0; a0 < kv.second.size(); a0 += (size_t)nmax) {
			Piece p;
			p.idx.assign(kv.second.begin() + a0, kv.second.begin() + std::min(kv.second.size(), a0 + (size_t)nmax));
			p.H = H; p.W = W; p.nbytes = per_target * (double)p.idx.size();
			if (!parts.back().empty() && acc + p.nbytes > budget) { parts.emplace_back(); acc = 0.0; }
			acc += p.nbytes;
			parts.back().push_back(std::move(p));
		}
	}
	return parts;
}

// ---- the plugin's rules on the result of one target's attempt (photometry.py:93-170; plugins.mask_outcome, stamps.py) ----------
struct Attempt {
	int32_t flags, status;                // of the device pass
	int64_t stamp[4];                     // the stamp the pass ran on
	int64_t limits[4];                    // the region that exists (stamps.clip_stamp)
	int32_t attempts_left;                // this attempt included (stamps.retry_limit at the first)
	double budget_flux;                   // the quick-break budget of a bright target, NaN for the others
	const uint8_t* mask; const double* sumimage; int32_t H, W;   // of this target
};

// Event codes (pipeline._EVENT_TEXT): 1 no flux above threshold, 2 / 3 minimum aperture, 4 too many masks, 5 an exception upstream
// (its kind in `kind`), 6 could not resize any further, 7 haloswitch quick break (the flux in `edge_flux`), 8 too many resizes,
// 9 no targets in mask
struct Decision {
	enum Outcome { STANDS, ERROR, RESIZE } outcome = STANDS;
	int32_t status = 0;                   // STANDS: the device's, ERROR: kStatusError
	bool moved = false;                   // the stamp grew (counts as a resize whatever the outcome); `stamp` is the new one
	int64_t stamp[4] = {0, 0, 0, 0};
	int32_t n_codes = 0, codes[4] = {0, 0, 0, 0};
	int32_t kind = 0;
	double edge_flux = 0.0;
	void log(int32_t code) { codes[n_codes++] = code; }
	Decision& end(Outcome o, int32_t st) { outcome = o; status = st; return *this; }
};

inline Decision decide_target(const Attempt& t)
{
	static const int side_bit[4] = {2, 4, 8, 16};      // down, up, left, right (stamps.SIDES)
	static const int side_sign[4] = {-1, +1, -1, +1};
	Decision d;
	const int32_t fl = t.flags, kind = fl >> 8;
	for (int k = 0; k < 4; ++k) d.stamp[k] = t.stamp[k];
	if ((fl & (1 | 32 | kEdgeBits)) == 0 && kind == 0) return d.end(Decision::STANDS, t.status);   // the common case: nothing to log, no edge touched
	// plugins.mask_outcome
	if (fl & 32) d.log(1);
	if (fl & 1) d.log((fl & (32 | 64)) ? 2 : 3);
	if (kind == 5) { d.log(4); return d.end(Decision::ERROR, kStatusError); }
	if ((kind >= 1 && kind <= 4) || kind == 7) { d.log(5); d.kind = kind; return d.end(Decision::ERROR, kStatusError); }   // an uncaught exception upstream (plugins._MASK_EXCEPTIONS)
	if (fl & kEdgeBits) {
		const int64_t* before = t.stamp;
		int64_t* after = d.stamp;
		for (int s = 0; s < 4; ++s) if (fl & side_bit[s]) after[s] += side_sign[s] * kResizeStep;
		// stamps.clip_stamp (growing a valid stamp cannot empty it)
		after[0] = std::max(after[0], t.limits[0]); after[2] = std::max(after[2], t.limits[2]);
		after[1] = std::min(after[1], t.limits[1]); after[3] = std::min(after[3], t.limits[3]);
		if (std::equal(before, before + 4, after)) {
			d.log(6);                              // "Could not resize stamp any further.": the attempt just made stands
		} else {
			d.moved = true;
			bool quick = false;
			if (t.budget_flux == t.budget_flux) {       // bright target (not NaN): stamps.quick_break_flux
				bool side_stuck[4], any = false;
				for (int s = 0; s < 4; ++s) { side_stuck[s] = (fl & side_bit[s]) && before[s] == after[s]; any = any || side_stuck[s]; }
				if (any) {
					std::vector<double> vals;
					const int H = t.H, W = t.W;
					for (int r = 0; r < H; ++r)
						for (int c = 0; c < W; ++c) {
							const bool edge = (side_stuck[0] && r == 0) || (side_stuck[1] && r == H - 1) || (side_stuck[2] && c == 0) || (side_stuck[3] && c == W - 1);
							if (edge && t.mask[r * W + c]) { const double v = t.sumimage[r * W + c]; vals.push_back(v == v ? v : 0.0); }
						}
					d.edge_flux = np_pairwise_sum(vals.data(), (int64_t)vals.size());
					quick = d.edge_flux > t.budget_flux;
				}
			}
			if (quick) { d.log(7); return d.end(Decision::ERROR, kStatusError); }
			if (t.attempts_left - 1 == 0) { d.log(8); return d.end(Decision::ERROR, kStatusError); }
			return d.end(Decision::RESIZE, 0);
		}
	}
	if (kind == 6) d.log(9);                           // "No targets in mask."
	return d.end(Decision::STANDS, t.status);
}

} // namespace frames_rules
