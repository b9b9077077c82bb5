# -*- coding: utf-8 -*-
"""
Designed LinPSF scenes and the one case table the device tests (``test_gpu_linpsf_classes.py``) and the CPU-only host test
(``test_linpsf_host.py``) share.

The fit kernels (``photometry_amd/csrc/linpsf.hip``, ``linpsf_mfma.hip``) decide on the device which kernel fits a target: from
the number of fitted stars, the knot intervals of the PRF grid the stars visit, the pixels inside their cut-off circles, the
length of the series.  The scenes of ``simulate.make_scene`` leave that to chance and always put the target first in its
catalogue.  Here a target is built BY DESIGN -- star count, the target's place in the fitted list, positions, a per-star motion
series -- and the class it must reach is restated on the host (:func:`plan_class`, from the rules of ``tp_linpsf_plan_kernel``,
``photometry_amd/csrc/linpsf_plan_rules.h``: ``test_linpsf_plan_host.py`` holds the two to each other without a GPU),
so that every row of :data:`CASES` names its class, the counters of ``tp_linpsf_last_counts`` that prove it, and the CPU test
checks the row's design facts before the GPU ever sees it.

Pixels are rendered with the pixel model of ``simulate.fill_cubes`` (pixel-integrated Gaussians of ``mag2flux`` fluxes plus
noise); the oracle (``oracle.linpsf.do_photometry``) fits them with the pixel-integrated PRF like the kernels.
"""

import numpy as np

# ---- constants of the kernels, restated (photometry_amd/csrc/linpsf_plan_rules.h, linpsf.hip; test_linpsf_plan_host.py compares) ----
MAX_STARS = 8            # kMaxStars: register-resident vector-ALU kernels
MFMA_STARS = 4           # kMfmaStars
MFMA_PIXELS = 256        # kMfmaPixels
MFMA_SPAN = 3            # kMfmaSpan
MFMA_SEGS = 8            # kMfmaSegs
MFMA_CAD_TILES = 256     # kMfmaCadTiles (4096 cadences)
MFMA_LDS_SMALL, MFMA_LDS_LARGE = 75776, 157696
MAX_ORIGINS = 36         # kMaxOrigins: more table origins per star -> the general direct kernel
MAX_MANY_STARS = 64
CUTOFF = 5.0

PRF_SEED = 7
_cache = {}


def prf_and_model(kind='spoc'):
	"""The PRF samples of the LinPSF tests (``prf_common.general_prf``) and the host model of them, built once."""
	if ('prf', kind) not in _cache:
		from photometry_amd import psf as hpsf
		from prf_common import general_prf
		prf = general_prf(kind)
		_cache[('prf', kind)] = (prf, hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow']))
	return _cache[('prf', kind)]


# --------------------------------------------------------------------------------------------------
# host restatement of the plan kernel
# --------------------------------------------------------------------------------------------------
def axis_origin(knots, pos):
	"""``axis_phase`` (linpsf_dev.h): the table origin (``first``) of a position along one axis and its phase in the knot
	interval; ``valid`` False for a NaN / absurd position.  Arrays in, arrays out."""
	knots = np.asarray(knots, dtype='float64')
	n = len(knots) - 4
	pos = np.asarray(pos, dtype='float64')
	with np.errstate(invalid='ignore'):
		valid = np.abs(pos) < 1e6
	p = np.where(valid, pos, 0.0)
	jstar = np.rint(p)
	x0 = (jstar - p) - 0.5
	l = np.clip(np.searchsorted(knots, x0, side='right') - 1, 4, n - 2)      # kn[l] <= x0 < kn[l + 1] on the even part
	phi = (x0 - knots[l]) / (knots[l + 1] - knots[l])
	first = (l - 3) - 9 * jstar.astype('int64')
	return first, phi, valid


def _interval_boxes(model, pos_row, pos_col):
	"""Per cadence: origin along x (columns, ``model.tx``) and y (rows, ``model.ty``) and whether both are valid."""
	ax, _, vx = axis_origin(model.tx, pos_col)
	by, _, vy = axis_origin(model.ty, pos_row)
	return ax, by, vx & vy


def intervals_visited(model, pos_row, pos_col, tile0=0, tile1=None):
	"""
	How many knot intervals per axis a star visits over the 16-cadence tiles ``[tile0, tile1)`` of its series: ``(na, nb)`` --
	``na`` along the first spline axis (columns), ``nb`` along the second (rows) -- as ``emit_segment`` counts them (highest
	minus lowest origin plus one over the cadences with a valid position; ``(0, 0)`` when there is none).
	"""
	pos_row, pos_col = np.asarray(pos_row, dtype='float64'), np.asarray(pos_col, dtype='float64')
	T = len(pos_row)
	k0, k1 = 16 * tile0, (T if tile1 is None else min(T, 16 * tile1))
	ax, by, ok = _interval_boxes(model, pos_row[k0:k1], pos_col[k0:k1])
	if not ok.any():
		return (0, 0)
	return (int(ax[ok].max() - ax[ok].min() + 1), int(by[ok].max() - by[ok].min() + 1))


def origin_count(model, pos_row, pos_col):
	"""Table origins of a star over the whole series (``StarPlan.nc``): the box of the origins it visits."""
	na, nb = intervals_visited(model, pos_row, pos_col)
	return na * nb


def on_stamp(pos_row, pos_col, H, W, cutoff=CUTOFF):
	"""Can the star's cut-off circle reach a pixel at some cadence (the plan kernel's pixel box of the star, clipped to the stamp)?"""
	pos_row, pos_col = np.asarray(pos_row, dtype='float64'), np.asarray(pos_col, dtype='float64')
	with np.errstate(invalid='ignore'):
		ok = (np.abs(pos_row) < 1e6) & (np.abs(pos_col) < 1e6)
	if not ok.any():
		return False
	jmin, jmax = np.floor(pos_col[ok] - cutoff).min(), np.ceil(pos_col[ok] + cutoff).max()
	imin, imax = np.floor(pos_row[ok] - cutoff).min(), np.ceil(pos_row[ok] + cutoff).max()
	return bool(max(jmin, 0) <= min(jmax, W - 1) and max(imin, 0) <= min(imax, H - 1))


def segments(model, pos_rows, pos_cols, limit=MFMA_SEGS):
	"""
	The greedy segmentation of the plan kernel: the series in 16-cadence tiles, a segment ends before the tile that would take a
	star beyond ``MFMA_SPAN`` knot intervals on an axis.  ``pos_rows`` / ``pos_cols``: ``(S, T)``.  Returns the list of
	``(tile0, tile1)`` or ``None`` when one tile alone goes beyond the span or more than ``limit`` (``MFMA_SEGS``) segments are needed.
	"""
	S, T = pos_rows.shape
	ntile = (T + 15) // 16
	lo = np.full((S, ntile, 2), 2**30)
	hi = np.full((S, ntile, 2), -2**30)
	for s in range(S):
		ax, by, ok = _interval_boxes(model, pos_rows[s], pos_cols[s])
		for t in range(ntile):
			m = ok[16 * t:16 * t + 16]
			if m.any():
				a, b = ax[16 * t:16 * t + 16][m], by[16 * t:16 * t + 16][m]
				lo[s, t] = (a.min(), b.min())
				hi[s, t] = (a.max(), b.max())
	segs, start = [], 0
	clo, chi = np.full((S, 2), 2**30), np.full((S, 2), -2**30)
	for t in range(ntile):
		nlo, nhi = np.minimum(clo, lo[:, t]), np.maximum(chi, hi[:, t])
		if np.any((nhi >= nlo) & (nhi - nlo + 1 > MFMA_SPAN)):
			if t == start:
				return None
			segs.append((start, t))
			start = t
			nlo, nhi = lo[:, t].copy(), hi[:, t].copy()
			if np.any((nhi >= nlo) & (nhi - nlo + 1 > MFMA_SPAN)):
				return None
		clo, chi = nlo, nhi
	segs.append((start, ntile))
	return segs if len(segs) <= limit else None


def _gray_rank4(g):
	g ^= g >> 2
	g ^= g >> 1
	return g & 15


def union_plan(pos_rows, pos_cols, H, W, cutoff=CUTOFF, with_keys=False):
	"""
	The union list of the matrix-core path: the pixels nearer than the cut-off to the rectangle a star's position sweeps, for any
	star on the stamp; ordered as the plan kernel orders them; cut into tiles of 16.  Returns ``(n_pix, tiles)`` with ``tiles[s]``
	the number of tiles star ``s`` touches (``None`` beyond ``MFMA_PIXELS`` pixels: no list is made); ``with_keys``: and the keys
	the list is ordered by, in raster order of their pixels (``pixel_key`` of linpsf_plan_rules.h).
	"""
	S = pos_rows.shape[0]
	reach, always = (cutoff + 1e-6)**2, (cutoff - 1e-6)**2
	ii, jj = np.meshgrid(np.arange(H, dtype='float64'), np.arange(W, dtype='float64'), indexing='ij')
	sig = np.zeros((H, W), dtype='int64')
	edge = np.zeros((H, W), dtype='int64')
	for s in range(S):
		if not on_stamp(pos_rows[s], pos_cols[s], H, W, cutoff):
			continue
		with np.errstate(invalid='ignore'):
			ok = (np.abs(pos_rows[s]) < 1e6) & (np.abs(pos_cols[s]) < 1e6)
		r0, r1, c0, c1 = pos_rows[s][ok].min(), pos_rows[s][ok].max(), pos_cols[s][ok].min(), pos_cols[s][ok].max()
		dr = np.maximum(0.0, np.maximum(r0 - ii, ii - r1))
		dc = np.maximum(0.0, np.maximum(c0 - jj, jj - c1))
		inside = dr * dr + dc * dc < reach
		fr = np.maximum(np.abs(ii - r0), np.abs(ii - r1))
		fc = np.maximum(np.abs(jj - c0), np.abs(jj - c1))
		sig |= inside.astype('int64') << s
		edge |= (inside & ~(fr * fr + fc * fc < always)).astype('int64') << s
	p = np.flatnonzero(sig.ravel())
	n_pix = len(p)
	if n_pix > MFMA_PIXELS:
		return (n_pix, None, None) if with_keys else (n_pix, None)
	sg, ed = sig.ravel()[p], edge.ravel()[p]
	keys = (_gray_rank4(sg.copy()) << 25) | ((ed != 0).astype('int64') << 24) | (ed << 20) | (sg << 16) | p
	rank = np.argsort(np.argsort(keys))
	tiles = [len(set((rank[(sg >> s) & 1 == 1] >> 4).tolist())) for s in range(S)]
	return (n_pix, tiles, keys) if with_keys else (n_pix, tiles)


def mfma_steps(na, nb):
	"""``mfma_steps`` (linpsf_common.h): matrix-instruction steps per (star, pixel tile); 2 x 2 intervals are packed into 9."""
	return 9 if (na, nb) == (2, 2) else (4 + na) + 2 * nb


def plan_class(model, pos_rows, pos_cols, H, W, path, cutoff=CUTOFF):
	"""
	Which kernel fits a target, by the rules of ``tp_linpsf_plan_kernel`` / ``linpsf_fit_impl`` on the SPOC grid:
	``{'cls': 'matrix' | 'poly' | 'direct' | 'many', 'segments': [...], 'n_pix': .., 'lds': [bytes per segment], 'shapes': ..}``.
	"""
	S, T = pos_rows.shape
	out = {'stars': S}
	if S > MAX_STARS:
		out['cls'] = 'many'
		return out
	live = [on_stamp(pos_rows[s], pos_cols[s], H, W, cutoff) for s in range(S)]
	nc = [origin_count(model, pos_rows[s], pos_cols[s]) if live[s] else 0 for s in range(S)]
	out['origins'] = nc
	fallback = 'direct' if max(nc + [0]) > MAX_ORIGINS else 'poly'
	out['cls'] = fallback
	if not (path == 1 and 1 <= S <= MFMA_STARS and H * W <= 65535 and T <= 16 * MFMA_CAD_TILES):
		return out
	segs = segments(model, pos_rows, pos_cols)
	out['segments'] = segs
	if segs is None:
		return out
	n_pix, tiles = union_plan(pos_rows, pos_cols, H, W, cutoff)
	out['n_pix'] = n_pix
	if tiles is None:
		return out
	shapes, lds = [], []
	for (t0, t1) in segs:
		sh = [intervals_visited(model, pos_rows[s], pos_cols[s], t0, t1) if live[s] else (0, 0) for s in range(S)]
		shapes.append(sh)
		lds.append(512 * sum(tiles[s] * mfma_steps(*sh[s]) for s in range(S) if sh[s][0] > 0))
	out['shapes'], out['lds'], out['tiles'] = shapes, lds, tiles
	if max(lds) > (MFMA_LDS_SMALL if S <= 1 else MFMA_LDS_LARGE):
		return out
	out['cls'] = 'matrix'
	return out


def expected_counts(classes, any_grid=False):
	"""The ``linpsf_last_counts`` dict a batch with these :func:`plan_class` results must leave."""
	c = {'matrix_core_targets': 0, 'matrix_core_segments': 0, 'vector_alu_polynomial_targets': 0, 'vector_alu_general_targets': 0,
		'many_star_targets': 0, 'matrix_core_targets_by_stars': [0, 0, 0, 0], 'matrix_core_segments_by_stars': [0, 0, 0, 0], 'any_grid_targets': 0}
	if any_grid:
		c['any_grid_targets'] = len(classes)
		return c
	for p in classes:
		if p['cls'] == 'matrix':
			c['matrix_core_targets'] += 1
			c['matrix_core_segments'] += len(p['segments'])
			c['matrix_core_targets_by_stars'][p['stars'] - 1] += 1
			c['matrix_core_segments_by_stars'][p['stars'] - 1] += len(p['segments'])
		elif p['cls'] == 'poly':
			c['vector_alu_polynomial_targets'] += 1
		elif p['cls'] == 'direct':
			c['vector_alu_general_targets'] += 1
		else:
			c['many_star_targets'] += 1
	return c


# --------------------------------------------------------------------------------------------------
# designed targets
# --------------------------------------------------------------------------------------------------
def snap(knots, pos):
	"""The position nearest to ``pos`` (below it by less than one knot interval) that sits in the MIDDLE of its knot interval."""
	_, phi, _ = axis_origin(knots, np.array([pos]))
	h = knots[5] - knots[4]
	return float(pos + (phi[0] - 0.5) * h)      # the phase falls as the position rises


def shape_motion(model, T, na, nb, rng, wobble=0.2):
	"""A jitter series ``(T, 2)`` (row, column) for a star snapped to the middle of its knot intervals that makes it visit exactly
	``na`` intervals along the columns and ``nb`` along the rows: whole steps of the knot spacing plus a wobble inside the interval."""
	hx, hy = model.tx[5] - model.tx[4], model.ty[5] - model.ty[4]
	k = np.arange(T)
	sa = (k % na) - (na // 2)
	sb = ((k // na) % nb) - (nb // 2)
	m = np.empty((T, 2))
	m[:, 0] = (sb + rng.uniform(-wobble, wobble, T)) * hy
	m[:, 1] = (sa + rng.uniform(-wobble, wobble, T)) * hx
	return m


def ring_positions(S, place, centre, radius=3.1, phase=0.4):
	"""``S`` star positions (row, column), the target at index ``place`` in the middle of the stamp and the others on a ring around it."""
	out = []
	j = 0
	for s in range(S):
		if s == place:
			out.append((centre[0] + 0.17, centre[1] - 0.21))
		else:
			a = phase + 2 * np.pi * j / max(S - 1, 1)
			out.append((centre[0] + radius * np.sin(a), centre[1] + radius * np.cos(a)))
			j += 1
	return out


def disc_positions(S, place, centre, radius=4.8):
	"""``S`` positions on a hexagonal lattice inside a disc around the target (for the many-star kernel: up to 64 stars nearer
	than 5 px to the target that are nowhere collinear as a whole); the lattice point nearest the centre is the target's."""
	d = np.sqrt(np.pi * radius**2 / (0.866 * S)) * 0.93
	while True:
		pts = []
		n = int(radius / d) + 2
		for a in range(-n, n + 1):
			for b in range(-n, n + 1):
				r, c = 0.866 * d * a + 0.07, d * (b + 0.5 * (a % 2)) - 0.11
				if r * r + c * c < radius * radius:
					pts.append((r * r + c * c, r, c))
		if len(pts) >= S:
			break
		d *= 0.98
	pts.sort()
	pts = pts[:S]
	order = [p for p in pts[1:]]
	order.insert(place, pts[0])
	return [(centre[0] + r, centre[1] + c) for (_, r, c) in order]


class Designed(object):
	"""A batch of designed targets: the attributes of ``simulate.Scene`` the LinPSF path reads, plus ``positions[i]``
	``(T, ncat_i, 2)`` -- what ``catalog_attime`` returns for target ``i`` -- and ``specs[i]`` (the design)."""

	def catalog_of(self, i):
		a, b = self.cat_offsets[i], self.cat_offsets[i + 1]
		return {k: v[a:b] for k, v in self.catalog.items()}


def design_target(model, S, place, T, H, W, shape=(1, 1), seed=0, layout='ring', motion=None, positions=None, rejected=2, target_tmag=9.5):
	"""
	One target by design.  ``S`` fitted stars with the target at ``place`` of the fitted list; ``layout`` 'ring' / 'disc' or explicit
	``positions`` (list of (row, column)); every star snapped to the middle of its knot intervals and moved by ``motion`` --
	``(T, 2)`` for all stars alike, ``(S, T, 2)`` per star, or None for :func:`shape_motion` of ``shape = (na, nb)``;
	``rejected`` stars the selection must drop (farther than 5 px / more than 5 mag fainter, alternately) lie in the catalogue
	ahead of the fitted ones, so that neither the catalogue index nor the fitted index of the target is 0.
	Returns a spec dict: ``cat`` (starid, tmag, row_stamp, column_stamp), ``pos`` ``(T, ncat, 2)``, ``fitted`` (catalogue rows of
	the fitted stars, in order), ``place``, ``flux`` (per catalogue star).
	"""
	rng = np.random.default_rng([seed, S, place, T])
	centre = ((H - 1) / 2.0, (W - 1) / 2.0)
	if positions is None:
		positions = ring_positions(S, place, centre) if layout == 'ring' else disc_positions(S, place, centre)
	base = np.array([(snap(model.ty, r), snap(model.tx, c)) for (r, c) in positions])
	if motion is None:
		motion = shape_motion(model, T, shape[0], shape[1], rng)
	motion = np.asarray(motion, dtype='float64')
	if motion.ndim == 2:
		motion = np.broadcast_to(motion[None], (S, T, 2))
	tmag = target_tmag + rng.uniform(0.3, 2.5, S)
	tmag[place] = target_tmag
	# catalogue: the rejected stars first, then the fitted ones in order
	rows, cols, mags, fitted = [], [], [], []
	for q in range(rejected):
		if q % 2 == 0:       # too far (but on the stamp): 5.5 px and more from the target
			a = 0.9 + 1.7 * q
			rows.append(base[place, 0] + 5.6 * np.sin(a))
			cols.append(base[place, 1] + 5.6 * np.cos(a))
			mags.append(target_tmag + 0.5)
		else:                # near, but more than 5 mag fainter
			rows.append(base[place, 0] + 1.3)
			cols.append(base[place, 1] - 2.2)
			mags.append(target_tmag + 5.5 + 0.1 * q)
	for s in range(S):
		fitted.append(len(rows))
		rows.append(base[s, 0])
		cols.append(base[s, 1])
		mags.append(tmag[s])
	ncat = len(rows)
	pos = np.empty((T, ncat, 2))
	pos[:, :, 0] = np.array(rows)[None, :]
	pos[:, :, 1] = np.array(cols)[None, :]
	common = motion[place]
	for c in range(ncat):
		pos[:, c, :] += motion[fitted.index(c)] if c in fitted else common
	return {'S': S, 'place': place, 'fitted': fitted, 'pos': pos,
		'cat': {'tmag': np.array(mags, dtype='float32'), 'row_stamp': np.array(rows, dtype='float32'), 'column_stamp': np.array(cols, dtype='float32')},
		'flux': 10**(-0.4 * (np.array(mags) - 20.451))}


def designed_scene(specs, T, H, W, seed=0, nan_fraction=0.004, sigma_psf=0.9, bkg=120.0, readnoise=10.0):
	"""The batch of the targets ``specs`` (from :func:`design_target`, same ``T``): catalogue, positions and the float32 cube."""
	from photometry_amd.simulate import _gauss_int
	rng = np.random.default_rng([seed, 777])
	s = Designed()
	Nt = len(specs)
	s.n_targets, s.n_cad, s.height, s.width, s.specs = Nt, T, H, W, specs
	row0 = rng.integers(0, 2048 - H, Nt)
	col0 = rng.integers(44, 44 + 2048 - W, Nt)
	s.stamps = np.column_stack((row0, row0 + H, col0, col0 + W)).astype('int32')
	s.target_starid = (np.arange(Nt, dtype='int64') + 1) * 1000
	offs, cols = [0], {k: [] for k in ('starid', 'tmag', 'row_stamp', 'column_stamp', 'row', 'column')}
	s.positions = []
	s.target_tmag = np.empty(Nt)
	s.target_pos_row, s.target_pos_column = np.empty(Nt), np.empty(Nt)
	images = np.empty((Nt, H, W, T), dtype='float32')
	rr, cc = np.arange(H, dtype='float64'), np.arange(W, dtype='float64')
	for i, sp in enumerate(specs):
		ncat = len(sp['cat']['tmag'])
		ids = s.target_starid[i] + 1 + np.arange(ncat, dtype='int64')
		tcat = sp['fitted'][sp['place']]
		ids[tcat] = s.target_starid[i]
		cols['starid'].append(ids)
		for k in ('tmag', 'row_stamp', 'column_stamp'):
			cols[k].append(sp['cat'][k])
		cols['row'].append((sp['cat']['row_stamp'] + row0[i]).astype('float32'))
		cols['column'].append((sp['cat']['column_stamp'] + col0[i]).astype('float32'))
		offs.append(offs[-1] + ncat)
		s.positions.append(sp['pos'])
		s.target_tmag[i] = sp['cat']['tmag'][tcat]
		s.target_pos_row[i] = sp['cat']['row_stamp'][tcat] + row0[i]
		s.target_pos_column[i] = sp['cat']['column_stamp'][tcat] + col0[i]
		signal = np.zeros((H, W, T))
		for c in range(ncat):
			pr, pc = sp['pos'][:, c, 0], sp['pos'][:, c, 1]
			ok = np.isfinite(pr) & np.isfinite(pc)
			gr = _gauss_int(rr[:, None], np.where(ok, pr, -100.0)[None, :], sigma_psf)
			gc = _gauss_int(cc[:, None], np.where(ok, pc, -100.0)[None, :], sigma_psf)
			signal += gr[:, None, :] * gc[None, :, :] * sp['flux'][c]
		img = signal + rng.standard_normal((H, W, T)) * np.sqrt(signal + bkg + readnoise**2)
		img = img.astype('float32')
		img[rng.random((H, W, T)) < nan_fraction] = np.nan
		images[i] = img
	s.cat_offsets = np.asarray(offs, dtype='int64')
	s.catalog = {k: np.concatenate(v) for k, v in cols.items()}
	s.images = images
	s.aperture = np.ones((Nt, H, W), dtype='int32')
	return s


def permute_catalog(scene, rng, place='random'):
	"""
	Reorders each target's slice of ``scene.catalog`` (call it before ``fill_cubes``: the cubes are rendered from ``star_params``,
	which it leaves alone, so only the ORDER of the catalogue changes): the target goes to the 'front', the 'middle', the 'end' of
	its slice or to a 'random' place; returns the permutation applied to the flat catalogue.  ``scene.positions`` (designed
	scenes) is reordered alike.
	"""
	perm = np.arange(len(scene.catalog['starid']))
	for i in range(scene.n_targets):
		a, b = int(scene.cat_offsets[i]), int(scene.cat_offsets[i + 1])
		n = b - a
		t = int(np.flatnonzero(scene.catalog['starid'][a:b] == scene.target_starid[i])[0])
		others = [j for j in rng.permutation(n) if j != t]
		at = {'front': 0, 'middle': n // 2, 'end': n - 1}.get(place, None)
		if at is None:
			at = int(rng.integers(0, n))
		others.insert(at, t)
		perm[a:b] = a + np.array(others)
		if getattr(scene, 'positions', None) is not None:
			scene.positions[i] = scene.positions[i][:, others, :]
	scene.catalog = {k: v[perm] for k, v in scene.catalog.items()}
	return perm


def add_rejected(scene, rng):
	"""Puts two stars the selection must drop -- one 5.5 px and more from the target, one more than 5 mag fainter -- AHEAD of
	every target in its catalogue slice of a ``simulate`` scene (before ``fill_cubes``; they carry no flux in the cubes)."""
	cols = {k: [] for k in scene.catalog}
	offs = [0]
	for i in range(scene.n_targets):
		a, b = int(scene.cat_offsets[i]), int(scene.cat_offsets[i + 1])
		t = a + int(np.flatnonzero(scene.catalog['starid'][a:b] == scene.target_starid[i])[0])
		r, c, m = (float(scene.catalog[k][t]) for k in ('row_stamp', 'column_stamp', 'tmag'))
		ang = rng.uniform(0, 2 * np.pi)
		extra = {'starid': [scene.target_starid[i] + 7, scene.target_starid[i] + 8], 'tmag': [m + 0.4, m + 5.6],
			'row_stamp': [r + 5.7 * np.sin(ang), r + 1.1], 'column_stamp': [c + 5.7 * np.cos(ang), c - 1.4]}
		extra['row'] = [x + scene.stamps[i, 0] for x in extra['row_stamp']]
		extra['column'] = [x + scene.stamps[i, 2] for x in extra['column_stamp']]
		for k in scene.catalog:
			cols[k].append(np.concatenate((np.asarray(extra[k], dtype=scene.catalog[k].dtype), scene.catalog[k][a:b])))
		offs.append(offs[-1] + (b - a) + 2)
	scene.catalog = {k: np.concatenate(v) for k, v in cols.items()}
	scene.cat_offsets = np.asarray(offs, dtype='int64')


def fit_inputs(scene):
	"""``select_stars`` and the position arrays ``(n_fit_stars, T)`` of a designed batch."""
	from photometry_amd import psf as hpsf
	sel, star_offsets, target_index = hpsf.select_stars(scene.catalog, scene.cat_offsets, scene.target_starid)
	pr = np.concatenate([p[:, :, 0].T for p in scene.positions])[sel]
	pc = np.concatenate([p[:, :, 1].T for p in scene.positions])[sel]
	return sel, star_offsets, target_index, np.ascontiguousarray(pr), np.ascontiguousarray(pc)


# --------------------------------------------------------------------------------------------------
# the case table
# --------------------------------------------------------------------------------------------------
def _drift(T, d_row, d_col):
	"""A linear drift ``(T, 2)`` of ``d_row`` / ``d_col`` knot intervals of the SPOC grid (1/9 px) over the series."""
	ramp = np.linspace(0.0, 1.0, T) if T > 1 else np.zeros(1)
	return np.stack((d_row * ramp / 9.0, d_col * ramp / 9.0), axis=1)


def _stairs(T, s_row, s_col):
	"""A staircase ``(T, 2)``: every 16-cadence tile stands still, ``s_row`` / ``s_col`` knot intervals beyond the tile before it.  With
	steps of 3 and more every tile is a segment of its own with ONE interval per axis, whatever area the whole series sweeps."""
	k = np.arange(T) // 16
	return np.stack((s_row * k / 9.0, s_col * k / 9.0), axis=1)


def _wide(T, seed, amp=0.42):
	"""Jitter of +-``amp`` px on both axes: 7 x 7 and more table origins, several knot intervals inside every 16 cadences."""
	return np.random.default_rng([seed, 99]).uniform(-amp, amp, (T, 2))


def _targets_shapes(model, T, H, W):
	out = []
	places = {1: [0, 0, 0, 0], 2: [1, 0, 1, 1], 3: [1, 2, 0, 2], 4: [1, 3, 2, 0]}
	for S in (1, 2, 3, 4):
		for q, shape in enumerate(((1, 1), (2, 2), (3, 3), (1, 3) if S % 2 else (3, 2))):
			out.append(design_target(model, S, places[S][q], T, H, W, shape=shape, seed=10 + q))
	return out


def _targets_segments(model, T, H, W):
	# (columns drift by so many knot intervals; the rows stay inside one)
	return [design_target(model, 1, 0, T, H, W, motion=_drift(T, 0, 0), seed=20),
		design_target(model, 2, 1, T, H, W, motion=_drift(T, 0, 4.0), seed=21),
		design_target(model, 1, 0, T, H, W, motion=_drift(T, 0, 16.0), seed=22),
		design_target(model, 2, 1, T, H, W, motion=_drift(T, 0, -16.0), seed=23),
		design_target(model, 1, 0, T, H, W, motion=_drift(T, 0, 17.5), seed=24),
		design_target(model, 2, 0, T, H, W, motion=_drift(T, 0, -17.5), seed=25)]


def _targets_short(model, T, H, W):
	return [design_target(model, 1, 0, T, H, W, seed=30), design_target(model, 2, 1, T, H, W, seed=31),
		design_target(model, 3, 1, T, H, W, seed=32), design_target(model, 3, 2, T, H, W, seed=33), design_target(model, 4, 3, T, H, W, seed=34),
		design_target(model, 6, 4, T, H, W, seed=35), design_target(model, 9, 5, T, H, W, seed=36, layout='disc')]


def _targets_long(model, T, H, W):
	m = _drift(T, 0, 1.0)
	return [design_target(model, 1, 0, T, H, W, motion=m, seed=40, rejected=3), design_target(model, 2, 1, T, H, W, motion=m, seed=41)]


def _union_positions(H, W):
	c = ((H - 1) / 2.0, (W - 1) / 2.0)
	return [(c[0] + 4.9 * np.sin(a), c[1] + 4.9 * np.cos(a)) for a in (0.3, 0.3 + 2 * np.pi / 3, 0.3 + 4 * np.pi / 3)]


def _targets_union(model, T, H, W, stairs):
	c = ((H - 1) / 2.0, (W - 1) / 2.0)
	ring = _union_positions(H, W)
	out = []
	for place in (1, 3):
		pos = list(ring)
		pos.insert(place, c)
		out.append(design_target(model, 4, place, T, H, W, positions=pos, motion=_stairs(T, *stairs), seed=50 + place))
	return out


def _targets_valu(model, T, H, W, wide):
	places = [0, 1, 1, 3, 2, 5, 3, 7]
	return [design_target(model, S, places[S - 1], T, H, W, shape=(2, 1), motion=(_wide(T, S) if wide else None), seed=60 + S) for S in range(1, 9)]


def _targets_many(model, T, H, W):
	return [design_target(model, 9, 0, T, H, W, layout='disc', seed=70), design_target(model, 33, 16, T, H, W, layout='disc', seed=71),
		design_target(model, 64, 63, T, H, W, layout='disc', seed=72)]


def _targets_anygrid(model, T, H, W):
	return [design_target(model, 2, 1, T, H, W, shape=(2, 2), seed=80), design_target(model, 5, 2, T, H, W, shape=(2, 2), seed=81),
		design_target(model, 12, 11, T, H, W, shape=(2, 2), seed=82, layout='disc')]


def _targets_mixed(model, T, H, W):
	"""Every class in one call, interleaved: 23 targets."""
	t = []
	t.append(design_target(model, 3, 1, T, H, W, shape=(2, 2), seed=100))
	t.append(design_target(model, 6, 5, T, H, W, seed=101))
	t.append(design_target(model, 1, 0, T, H, W, motion=_drift(T, 0, 5.0), seed=102))
	t.append(design_target(model, 9, 4, T, H, W, layout='disc', seed=103))
	t.append(design_target(model, 2, 1, T, H, W, motion=_wide(T, 104), seed=104))
	t.append(design_target(model, 4, 3, T, H, W, shape=(1, 3), seed=105))
	t.append(design_target(model, 2, 0, T, H, W, shape=(3, 3), seed=106))
	t.append(design_target(model, 8, 7, T, H, W, seed=107))
	t.append(design_target(model, 3, 2, T, H, W, motion=_drift(T, -4.0, 7.0), seed=108))
	t.append(design_target(model, 1, 0, T, H, W, shape=(3, 3), seed=109, rejected=4))
	t.append(design_target(model, 5, 2, T, H, W, motion=_wide(T, 110), seed=110))
	t.append(design_target(model, 4, 0, T, H, W, shape=(2, 2), seed=111))
	t.append(design_target(model, 14, 13, T, H, W, layout='disc', seed=112))
	t.append(design_target(model, 2, 1, T, H, W, motion=_drift(T, 0, 7.5), seed=113))
	t.append(design_target(model, 3, 0, T, H, W, motion=_wide(T, 114), seed=114))
	t.append(design_target(model, 7, 3, T, H, W, shape=(2, 1), seed=115))
	t.append(design_target(model, 1, 0, T, H, W, seed=116))
	t.append(design_target(model, 4, 2, T, H, W, motion=_drift(T, 5.0, 0.0), seed=117))
	t.append(design_target(model, 3, 1, T, H, W, shape=(3, 2), seed=118))
	t.append(design_target(model, 1, 0, T, H, W, motion=_wide(T, 119), seed=119))
	t.append(design_target(model, 2, 1, T, H, W, shape=(2, 2), seed=120))
	t.append(design_target(model, 5, 4, T, H, W, shape=(2, 2), seed=121))
	t.append(design_target(model, 4, 1, T, H, W, shape=(3, 3), seed=122))
	return t


# ---- data edges: one batch (a matrix-core class on path 1 = a fit2 class on path 0, fit2<8,5> and the many-star kernel on both) ----
EDGE_T, EDGE_H, EDGE_W = 33, 13, 13


def _targets_edges(model, T, H, W, edge):
	"""The batch of the data-edge cases: 2, 3, 3, 6 and 10 fitted stars, the target never first; ``edge`` says what is done to the
	star positions (the pixel edges are applied by :func:`apply_pixel_edge`)."""
	base = [(2, 1), (3, 1), (3, 2), (6, 3), (10, 9)]
	out = []
	for q, (S, place) in enumerate(base):
		# ('nan_segment': a staircase of 3 knot intervals per tile of cadences, so that every tile is a segment of its own)
		sp = design_target(model, S, place, T, H, W, shape=(2, 2), seed=200 + q, layout='disc' if S > 8 else 'ring',
			motion=_stairs(T, 0, 3) if edge == 'nan_segment' else None)
		nb = sp['fitted'][(place + 1) % S]         # a neighbour of the target (catalogue row)
		tg = sp['fitted'][place]
		if edge == 'leaves':        # from the third tile of cadences on the neighbour is 30 px off the stamp
			sp['pos'][32:, nb, 1] += 30.0
			sp['pos'][32:, nb, 1] = [snap(model.tx, v) for v in sp['pos'][32:, nb, 1]]
		elif edge == 'never':       # catalogue position beside the target, never nearer than the cut-off to a pixel
			sp['pos'][:, nb, 0] += 40.0
		elif edge == 'nan_row':
			sp['pos'][[0, 7, T - 1], nb, 0] = np.nan
		elif edge == 'nan_col':
			sp['pos'][[0, 9, T - 1], nb if q % 2 else tg, 1] = np.nan
		elif edge == 'nan_both':
			sp['pos'][[0, 11, 12, T - 1], nb, :] = np.nan
			sp['pos'][[3], tg, :] = np.nan
		elif edge in ('nan_stretch', 'nan_segment'):  # no valid position of the neighbour in the whole second tile of cadences
			sp['pos'][16:32, nb, :] = np.nan
		out.append(sp)
	return out


def apply_pixel_edge(scene, edge):
	"""The pixel-side data edges, applied to the rendered cube."""
	im = scene.images
	if edge == 'last_frame_nan':
		im[:, :, :, -1] = np.nan
	elif edge == 'last_frame_centre_nan':
		for i in range(scene.n_targets):
			r, c = int(round(scene.target_pos_row[i] - scene.stamps[i, 0])), int(round(scene.target_pos_column[i] - scene.stamps[i, 2]))
			im[i, r - 1:r + 2, c - 1:c + 2, -1] = np.nan
	elif edge == 'nan_pixel_column':
		im[:, :, scene.width // 2 + 1, :] = np.nan


#: name -> dict(cls: the class the row is built to reach; T, H, W; targets: builder(model, T, H, W); paths; kind / cutoff of the PRF grid;
#: counts: {path: the linpsf_last_counts fields and values that prove the class}; facts: design facts the host test asserts;
#: pos_edge / pixel_edge / subtract / pitches: the data edges).  ``counts`` are written out here and ALSO derived from
#: :func:`plan_class` in test_linpsf_host.py: a row whose design does not reach its class fails on the CPU.
def _c(**kw):
	c = {'matrix_core_targets': 0, 'matrix_core_segments': 0, 'vector_alu_polynomial_targets': 0, 'vector_alu_general_targets': 0,
		'many_star_targets': 0, 'matrix_core_targets_by_stars': [0, 0, 0, 0], 'matrix_core_segments_by_stars': [0, 0, 0, 0], 'any_grid_targets': 0}
	c.update(kw)
	return c


_EDGE_COUNTS = {0: _c(vector_alu_polynomial_targets=4, many_star_targets=1),
	1: _c(matrix_core_targets=3, matrix_core_segments=3, matrix_core_targets_by_stars=[0, 1, 2, 0], matrix_core_segments_by_stars=[0, 1, 2, 0],
		vector_alu_polynomial_targets=1, many_star_targets=1)}

CASES = {
	# 1. matrix-core classes, one segment: S = 1..4 x (na, nb) = (1,1), (2,2), (3,3), mixed.  The three-star (3,3) target's coefficient
	#    image is 3 stars x tiles x 13 steps x 512 B (facts: lds_over_small) -> beyond kMfmaLdsSmall, inside kMfmaLdsLarge; the
	#    four-star (3,3) target's is beyond kMfmaLdsLarge too and leaves the matrix cores (facts: lds_over_large)
	'matrix_shapes': dict(cls='matrix core, 1 segment, 1-4 stars', T=32, H=13, W=13, targets=_targets_shapes, paths=(0, 1),
		counts={0: _c(vector_alu_polynomial_targets=16),
			1: _c(matrix_core_targets=15, matrix_core_segments=15, matrix_core_targets_by_stars=[4, 4, 4, 3], matrix_core_segments_by_stars=[4, 4, 4, 3],
				vector_alu_polynomial_targets=1)},
		facts=dict(shapes=[(1, 1), (2, 2), (3, 3), (1, 3), (1, 1), (2, 2), (3, 3), (3, 2)] * 2, lds_over_small=10, lds_over_large=14)),
	# 2. segments: 1, 2, 8 segments; a ninth leaves the matrix cores (333 cadences = 21 tiles)
	'segments_333': dict(cls='matrix core, 1 / 2 / 8 segments; 9 -> vector ALU', T=333, H=11, W=11, targets=_targets_segments, paths=(0, 1),
		counts={0: _c(vector_alu_polynomial_targets=6),
			1: _c(matrix_core_targets=4, matrix_core_segments=19, matrix_core_targets_by_stars=[2, 2, 0, 0], matrix_core_segments_by_stars=[9, 10, 0, 0],
				vector_alu_polynomial_targets=2)},
		facts=dict(n_segments=[1, 2, 8, 8, 9, 9])),
	'tail_1': dict(cls='series of 1 cadence', T=1, H=11, W=11, targets=_targets_short, paths=(0, 1), counts='short'),
	'tail_15': dict(cls='series of 15 cadences', T=15, H=11, W=11, targets=_targets_short, paths=(0, 1), counts='short'),
	'tail_16': dict(cls='series of 16 cadences', T=16, H=11, W=11, targets=_targets_short, paths=(0, 1), counts='short'),
	'tail_17': dict(cls='series of 17 cadences', T=17, H=11, W=11, targets=_targets_short, paths=(0, 1), counts='short'),
	'cadences_4096': dict(cls='4096 cadences: still on the matrix cores', T=4096, H=7, W=7, targets=_targets_long, paths=(1,),
		counts={1: _c(matrix_core_targets=2, matrix_core_segments=2, matrix_core_targets_by_stars=[1, 1, 0, 0], matrix_core_segments_by_stars=[1, 1, 0, 0])}),
	'cadences_4097': dict(cls='4097 cadences: beyond kMfmaCadTiles -> vector ALU', T=4097, H=7, W=7, targets=_targets_long, paths=(1,),
		counts={1: _c(vector_alu_polynomial_targets=2)}),
	# 3. union list: four stars on a 21 x 21 stamp, the neighbours 4.9 px from the target at 120 degrees; a staircase motion widens
	#    the area their cut-off circles sweep to 255 pixels (matrix cores, three segments of one knot interval: the coefficient image
	#    stays inside kMfmaLdsLarge, which a drift's 3 x 3 intervals would not) and to 257 (vector ALUs; 99 origins: the direct kernel)
	'union_under': dict(cls='matrix core, union list just under 256 pixels', T=48, H=21, W=21, targets=lambda m, T, H, W: _targets_union(m, T, H, W, UNION_STAIRS_UNDER), paths=(0, 1),
		counts={0: _c(vector_alu_general_targets=2),
			1: _c(matrix_core_targets=2, matrix_core_segments=6, matrix_core_targets_by_stars=[0, 0, 0, 2], matrix_core_segments_by_stars=[0, 0, 0, 6])},
		facts=dict(n_pix=[255, 255])),
	'union_over': dict(cls='union list over 256 pixels -> vector ALU', T=48, H=21, W=21, targets=lambda m, T, H, W: _targets_union(m, T, H, W, UNION_STAIRS_OVER), paths=(1,),
		counts={1: _c(vector_alu_general_targets=2)}, facts=dict(n_pix=[257, 257])),
	# 4. vector-ALU classes
	'valu_1to8': dict(cls='fit2<1,0> <2,2> <3,3> <4,4> <8,5>', T=24, H=13, W=13, targets=lambda m, T, H, W: _targets_valu(m, T, H, W, False), paths=(0,),
		counts={0: _c(vector_alu_polynomial_targets=8)}),
	'direct_1to8': dict(cls='fit_direct<2,0> <4,3> <8,5>', T=24, H=13, W=13, targets=lambda m, T, H, W: _targets_valu(m, T, H, W, True), paths=(0, 1),
		counts={0: _c(vector_alu_general_targets=8), 1: _c(vector_alu_general_targets=8)}, facts=dict(origins_over=36)),
	# 5. many-star kernel
	'many': dict(cls='many-star kernel, 9 / 33 / 64 stars', T=6, H=21, W=21, targets=_targets_many, paths=(0, 1),
		counts={0: _c(many_star_targets=3), 1: _c(many_star_targets=3)}),
	# 6. any-grid kernels
	'anygrid_rect': dict(cls='any-grid kernels, rect grid', T=10, H=13, W=13, targets=_targets_anygrid, paths=(1,), kind='rect', cutoff=5,
		counts={1: _c(any_grid_targets=3)}),
	'anygrid_nocut': dict(cls='any-grid kernels, SPOC grid without a cut-off', T=10, H=13, W=13, targets=_targets_anygrid, paths=(1,), kind='spoc', cutoff=None,
		counts={1: _c(any_grid_targets=3)}),
	# 7. every class in one call
	'mixed': dict(cls='every class in one call', T=40, H=15, W=15, targets=_targets_mixed, paths=(0, 1), counts='derived'),
}
UNION_STAIRS_UNDER, UNION_STAIRS_OVER = (5, 3), (5, 4)     # knot intervals per tile of cadences along the rows / the columns

# 8. data edges
for _e in ('leaves', 'never', 'nan_row', 'nan_col', 'nan_both', 'nan_stretch', 'nan_segment'):
	CASES['edge_' + _e] = dict(cls='data edge: star position (' + _e + ')', T=EDGE_T, H=EDGE_H, W=EDGE_W, paths=(0, 1), counts='derived', singular=(_e == 'never'),
		targets=(lambda e: (lambda m, T, H, W: _targets_edges(m, T, H, W, e)))(_e))
for _e in ('last_frame_nan', 'last_frame_centre_nan', 'nan_pixel_column', 'subtract', 'pitches'):
	CASES['edge_' + _e] = dict(cls='data edge: ' + _e, T=EDGE_T, H=EDGE_H, W=EDGE_W, paths=(0, 1), counts=_EDGE_COUNTS, pixel_edge=_e,
		targets=lambda m, T, H, W: _targets_edges(m, T, H, W, None))

#: the row's short series share one expectation per path: 1-4 stars on the matrix cores (path 1), 6 on fit2<8,5>, 9 on the many-star kernel
_SHORT_COUNTS = {0: _c(vector_alu_polynomial_targets=6, many_star_targets=1),
	1: _c(matrix_core_targets=5, matrix_core_segments=5, matrix_core_targets_by_stars=[1, 1, 2, 1], matrix_core_segments_by_stars=[1, 1, 2, 1],
		vector_alu_polynomial_targets=1, many_star_targets=1)}


def build_case(name):
	"""The scene of a row (built once per process) with its fit inputs."""
	if ('case', name) in _cache:
		return _cache[('case', name)]
	row = CASES[name]
	_, model = prf_and_model('spoc')      # the designs are made on the SPOC knots; the any-grid rows only need SOME motion
	T, H, W = row['T'], row['H'], row['W']
	specs = row['targets'](model, T, H, W)
	scene = designed_scene(specs, T, H, W, seed=sum(map(ord, name)))
	if row.get('pixel_edge'):
		apply_pixel_edge(scene, row['pixel_edge'])
	sel, star_offsets, target_index, pos_row, pos_col = fit_inputs(scene)
	case = {'name': name, 'row': row, 'scene': scene, 'sel': sel, 'star_offsets': star_offsets, 'target_index': target_index,
		'pos_row': pos_row, 'pos_col': pos_col}
	if row.get('pixel_edge') == 'subtract':
		# one float32 value per target and cadence, varying over the cadences, in a plane whose pitch exceeds n_cad; the cube carries it
		rng = np.random.default_rng(5)
		pitch = T + 7
		plane = np.full((scene.n_targets, pitch), np.float32(-7777.0))
		plane[:, :T] = (90.0 + 25.0 * rng.random((scene.n_targets, T))).astype('float32')
		case['subtract'] = plane.astype('float32')
		scene.images_raw = (scene.images + case['subtract'][:, None, None, :T]).astype('float32')
	_cache[('case', name)] = case
	return case


def case_classes(case, path):
	"""The :func:`plan_class` of every target of a row on the SPOC grid."""
	_, model = prf_and_model('spoc')
	so = case['star_offsets']
	s = case['scene']
	return [plan_class(model, case['pos_row'][so[i]:so[i + 1]], case['pos_col'][so[i]:so[i + 1]], s.height, s.width, path) for i in range(s.n_targets)]


def case_counts(case, path):
	"""The counters the row asserts on ``path``: written in the row, or (``'derived'``) from the host restatement of the plan."""
	row = case['row']
	counts = row['counts']
	if counts == 'short':
		return _SHORT_COUNTS[path]
	if counts == 'derived' or counts[path] == 'derived':
		return expected_counts(case_classes(case, path))
	return counts[path]


# --------------------------------------------------------------------------------------------------
# oracle and comparison
# --------------------------------------------------------------------------------------------------
def oracle_images(case, i):
	"""The cube the oracle fits for target ``i``: with ``subtract`` the float32 difference, which is what configs[4] hands it."""
	s = case['scene']
	if 'subtract' in case:
		T = s.n_cad
		return s.images_raw[i] - case['subtract'][i, :T][None, None, :]
	return s.images[i]


def oracle_case(case):
	"""``oracle.linpsf.do_photometry`` of every target of a row (once per process)."""
	if 'oracle' in case:
		return case['oracle']
	from oracle import psf as opsf, linpsf as olin
	row, s = case['row'], case['scene']
	prf, _ = prf_and_model(row.get('kind', 'spoc'))
	refs = []
	for i in range(s.n_targets):
		cat = s.catalog_of(i)
		p = opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(s.stamps[i]))
		refs.append(olin.do_photometry(oracle_images(case, i), p, cat, s.target_starid[i], s.positions[i], tuple(s.stamps[i]),
			s.target_pos_row[i], s.target_pos_column[i], s.aperture[i], cutoff_radius=row.get('cutoff', 5)))
	case['oracle'] = refs
	return refs


def compare_target(res, i, star_offsets, ref, T, label=''):
	"""One target of a device result (host dict of ``LinPSFResult.to_host()``) against the oracle's: flux, fluxes_mean, contamination,
	status, flux_err NaN -- the tolerances of test_gpu_linpsf.py -- and ``fluxes_all`` of EVERY fitted star per cadence."""
	a, b = int(star_offsets[i]), int(star_offsets[i + 1])
	scale = np.nanmax(np.abs(ref['flux']))
	msg = f'{label} target {i}'
	np.testing.assert_allclose(res['flux'][i][:T], ref['flux'], rtol=1e-8, atol=1e-9 * scale, err_msg=msg + ' flux')
	assert np.all(np.isnan(res['flux_err'][i][:T])), msg
	assert int(res['status'][i]) == ref['status'], (msg, int(res['status'][i]), ref['status'])
	np.testing.assert_allclose(res['contamination'][i], ref['contamination'], rtol=1e-7, atol=1e-11, err_msg=msg + ' contamination')
	np.testing.assert_allclose(res['fluxes_mean'][a:b], ref['fluxes_mean'], rtol=1e-8, atol=1e-9 * scale, err_msg=msg + ' fluxes_mean')
	# every fitted star, every cadence, on the scale of the largest fitted flux of the target
	fscale = np.nanmax(np.abs(ref['fluxes_all']))
	np.testing.assert_allclose(res['fluxes_all'][a:b, :T], ref['fluxes_all'].T, rtol=1e-8, atol=1e-9 * fscale, err_msg=msg + ' fluxes_all')


def run_case(ctx, case, path, targets=None, pitches=None):
	"""``engine.linpsf_fit`` of a row (or of the targets ``targets`` of it as a batch of their own) on ``path``; returns the host
	result dict, the counters and the star offsets of the call.  ``pitches = (pos_pitch, out_pitch, t_pitch)``: padded arrays,
	the padding filled with a sentinel."""
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	row, s = case['row'], case['scene']
	_, model = prf_and_model(row.get('kind', 'spoc'))
	T = s.n_cad
	idx = np.arange(s.n_targets) if targets is None else np.asarray(targets)
	so = case['star_offsets']
	stars = np.concatenate([np.arange(so[i], so[i + 1]) for i in idx])
	offs = np.concatenate(([0], np.cumsum([so[i + 1] - so[i] for i in idx]))).astype('int64')
	pos_row, pos_col = case['pos_row'][stars], case['pos_col'][stars]
	images = (s.images_raw if 'subtract' in case else s.images)[idx]
	sentinel = -12345.0
	out = None
	if pitches is not None:
		pp, op, tp = pitches
		pr = np.full((len(stars), pp), sentinel)
		pc = np.full((len(stars), pp), sentinel)
		pr[:, :T], pc[:, :T] = pos_row, pos_col
		pos_row, pos_col = pr, pc
		cube = DeviceCube(ctx, len(idx), T, s.height, s.width, t_pitch=tp)
		padded = np.full((len(idx), s.height, s.width, tp), np.float32(sentinel))
		padded[..., :T] = images
		cube.data = ctx.array(padded)      # the padded cube as it is (DeviceCube.from_host packs to its own pitch)
		out = engine.LinPSFResult(ctx, len(idx), len(stars), op)
		out.flux = ctx.array(np.full((len(idx), op), sentinel))
		out.flux_err = ctx.array(np.full((len(idx), op), sentinel))
		out.fluxes_all = ctx.array(np.full((len(stars), op), sentinel))
	else:
		cube = DeviceCube.from_host(ctx, np.ascontiguousarray(images))
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps[idx])))
	sub = ctx.array(np.ascontiguousarray(case['subtract'][idx])) if 'subtract' in case else None
	engine.linpsf_set_path(ctx, path)
	try:
		dev = engine.linpsf_fit(ctx, cube, coef, ctx.array(model.tx), ctx.array(model.ty), ctx.array(offs), ctx.array(case['target_index'][idx]),
			ctx.array(np.ascontiguousarray(pos_row)), ctx.array(np.ascontiguousarray(pos_col)), int(np.diff(offs).max()),
			cutoff_radius=row.get('cutoff', 5), subtract=sub, out=out)
		res = dev.to_host()
		counts = engine.linpsf_last_counts(ctx)
	finally:
		engine.linpsf_set_path(ctx, 1)
	if pitches is not None:
		res['cube_after'] = cube.data.to_host()
		res['cube_before'] = padded
	return res, counts, offs


def run_and_compare(ctx, case, path):
	"""Runs a row on ``path``, asserts its counters exactly and compares EVERY target with the oracle in full."""
	refs = oracle_case(case)
	res, counts, offs = run_case(ctx, case, path)
	assert counts == case_counts(case, path), (case['name'], path, counts, case_counts(case, path))
	s = case['scene']
	for i in range(s.n_targets):
		assert refs[i]['nstars'] == offs[i + 1] - offs[i] and refs[i]['staridx'] == case['target_index'][i]
		compare_target(res, i, offs, refs[i], s.n_cad, label=f"{case['name']} path {path}")
	return res, counts
