# -*- coding: utf-8 -*-
"""Shared helpers of the K2P2 parity tests (host-sim on CPU, HIP kernel on GPU)."""
import os
import ctypes
import functools
import subprocess
import numpy as np
from oracle import aperture as oap, k2p2 as ok2p2, sumimage as osum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM_SRC = os.path.join(ROOT, 'tests', 'hostsim', 'k2p2_hostsim.cpp')
HOSTSIM_DIR = os.path.join(ROOT, 'tests', 'hostsim', 'build')


@functools.lru_cache(maxsize=None)
def build_hostsim():
	"""The host build of photometry_amd/csrc/k2p2_core.h (tests/hostsim/k2p2_hostsim.cpp), compiled and loaded.  With
	``K2P2_HOSTSIM_COVERAGE=1`` in the environment the build is instrumented (``-O0 --coverage``) for the branch measurement that
	tests/test_k2p2_edges_host.py describes; the tests themselves are the same.  Built once per process: the test modules share it (and
	an instrumented build keeps one set of counters)."""
	os.makedirs(HOSTSIM_DIR, exist_ok=True)
	cov = os.environ.get('K2P2_HOSTSIM_COVERAGE', '') == '1'
	out = os.path.join(HOSTSIM_DIR, 'k2p2_hostsim_cov.so' if cov else 'k2p2_hostsim.so')
	opt = ['-O0', '--coverage', '-dumpbase', 'k2p2_hostsim_cov'] if cov else ['-O2']
	subprocess.run(['g++'] + opt + ['-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-I' + os.path.dirname(HOSTSIM_SRC), '-o', out, HOSTSIM_SRC], check=True, cwd=HOSTSIM_DIR)
	lib = ctypes.CDLL(out)
	lib.hostsim_k2p2.restype = ctypes.c_int
	lib.hostsim_k2p2_shared_bytes.restype = ctypes.c_longlong
	return lib


def lds_resident(H, W):
	"""Does a stamp of ``H x W`` pixels take the LDS-resident mask kernel (work arrays up to 160 KiB, k2p2.hip) rather than the one on HBM scratch?"""
	return build_hostsim().hostsim_k2p2_shared_bytes(ctypes.c_int(H*W)) <= 160*1024


def run_hostsim(lib, s, S, cut_override=None):
	Nt, H, W = s.n_targets, s.height, s.width
	c = s.catalog
	f32 = lambda a: np.ascontiguousarray(a, dtype='float32') # noqa: E731
	arrs = dict(S=np.ascontiguousarray(S, dtype='float64'), off=np.ascontiguousarray(s.cat_offsets, dtype='int64'),
		ccs=f32(c['column_stamp']), crs=f32(c['row_stamp']), tm=f32(c['tmag']), cc=f32(c['column']), cr=f32(c['row']),
		sid=np.ascontiguousarray(c['starid'], dtype='int64'), tr=np.ascontiguousarray(s.target_pos_row, dtype='float64'),
		tc=np.ascontiguousarray(s.target_pos_column, dtype='float64'), tt=np.ascontiguousarray(s.target_tmag, dtype='float64'),
		tsid=np.ascontiguousarray(s.target_starid, dtype='int64'), st=np.ascontiguousarray(s.stamps, dtype='int32'),
		ap=np.ascontiguousarray(s.aperture, dtype='int32'))
	out = dict(mask=np.zeros((Nt, H, W), dtype='uint8'), status=np.zeros(Nt, dtype='int32'), flags=np.zeros(Nt, dtype='int32'),
		contamination=np.zeros(Nt), diag=np.zeros((Nt, 8)), cat_in_mask=np.zeros(max(len(c['starid']), 1), dtype='uint8'))
	p = lambda a: a.ctypes.data_as(ctypes.c_void_p) # noqa: E731
	co = None if cut_override is None else p(np.ascontiguousarray(cut_override, dtype='float64'))
	lib.hostsim_k2p2(ctypes.c_int(Nt), ctypes.c_int(H), ctypes.c_int(W), p(arrs['S']), p(arrs['off']), p(arrs['ccs']), p(arrs['crs']),
		p(arrs['tm']), p(arrs['cc']), p(arrs['cr']), p(arrs['sid']), p(arrs['tr']), p(arrs['tc']), p(arrs['tt']), p(arrs['tsid']),
		p(arrs['st']), p(arrs['ap']), co, ctypes.c_double(0.8),
		p(out['mask']), p(out['status']), p(out['flags']), p(out['contamination']), p(out['diag']), p(out['cat_in_mask']))
	return out


def make_cases(kind, seed):
	"""Seeded scenes that exercise the different K2P2 branches."""
	from photometry_amd import simulate
	if kind == 'faint15':
		s = simulate.make_scene(48, 120, 15, 15, seed=seed)
	elif kind == 'small11':
		s = simulate.make_scene(32, 60, 11, 11, seed=seed)
	elif kind == 'crowded':
		s = simulate.make_scene(32, 100, 21, 17, seed=seed, max_neighbours=5, neighbour_tmag_range=(8.0, 13.0))
	elif kind == 'bright':
		s = simulate.make_scene(24, 150, 15, 15, seed=seed, tmag_range=(4.0, 7.5), neighbour_tmag_range=(6.0, 9.0))
	elif kind == 'tiny':
		s = simulate.make_scene(12, 40, 6, 7, seed=seed, max_neighbours=1)
	elif kind == 'wide':
		# a resized stamp of a crowded field: a dozen clusters, several of them at the stamp's edges and corners -- the per-cluster
		# passes of the mask builder run over windows around each cluster (k2p2_core.h: struct Win)
		s = simulate.make_scene(20, 60, 29, 33, seed=seed, max_neighbours=14, neighbour_tmag_range=(7.5, 13.5))
	elif kind == 'huge':
		# blended very bright stars on a 100 x 96 stamp: ONE cluster of several thousand pixels split by the watershed -- more ranks
		# than the three summary words of the flood's bit set hold (3 072): the scanning path of k2p2_core.h::watershed
		s = simulate.make_scene(3, 8, 100, 96, seed=seed, tmag_range=(1.0, 2.0), max_neighbours=2, neighbour_tmag_range=(1.0, 2.5), sigma_psf=7.0)
	elif kind == 'large':
		# beyond the LDS-resident mask builder (about 54 x 54 pixels): the work arrays live in HBM
		s = simulate.make_scene(5, 24, 62, 58, seed=seed, tmag_range=(4.0, 6.0), max_neighbours=6, neighbour_tmag_range=(6.0, 10.0), sigma_psf=1.6)
	else:
		raise ValueError(kind)
	simulate.fill_cubes(s, nan_fraction=0.002)
	S = osum.sumimage_batch(s.images, s.quality)
	rng = np.random.default_rng(seed)
	if kind == 'bright':
		# emulate saturated bleed columns
		for i in range(s.n_targets):
			c = int(round(s.star_params[i, 0, 1])); r = int(round(s.star_params[i, 0, 0]))
			sat = 0.6*np.nanmax(S[i])
			for rr in range(max(r-5, 0), min(r+6, s.height)):
				S[i, rr, c] = sat*(1 + 0.001*np.sin(rr))
	# a few degenerate sum images
	if s.n_targets >= 12:
		S[1][:] = np.nan                       # no flux at all -> K2P2NoFlux -> ERROR
		S[2][:] = -np.abs(S[2])                # no positive flux -> ERROR
		S[3][:] = 5.0                          # constant -> bandwidth 0 -> ERROR
		S[4][S[4] > np.nanpercentile(S[4], 30)] = np.nan   # most pixels never observed
		S[5][2, 3] = np.nan
		S[6][:] = np.abs(rng.normal(10, 1e-3, S[6].shape))  # pure noise, no star
		# target far from stamp centre (still inside), and on the edge
		s.target_pos_row[7] = s.stamps[7, 0] + 0.4
		s.target_pos_column[7] = s.stamps[7, 2] + s.width - 1.2
		# catalog empty for target 8
	return s, S


def oracle_batch(s, S, cut_override=None):
	out = []
	for i in range(s.n_targets):
		cat = s.catalog_of(i)
		kw = {}
		try:
			if cut_override is not None:
				c = np.column_stack((cat['column_stamp'], cat['row_stamp'], cat['tmag']))
				try:
					mm, info = ok2p2.k2p2FixFromSum(S[i], catalog=c, cut_override=cut_override[i], full_output=True, **oap.K2P2_SETTINGS)
					mm = None if mm is None else np.asarray(mm, dtype=bool)
				except ok2p2.K2P2NoStars:
					mm = None
				kw['masks'] = mm
			r = oap.do_photometry(S[i], s.images[i], s.images_err[i], s.backgrounds[i], tuple(s.stamps[i]),
				s.target_pos_row[i], s.target_pos_column[i], s.target_tmag[i], s.target_starid[i], cat,
				# bit 1 of BasePhotometry.aperture = finite sum image (BasePhotometry.py:1043)
				s.aperture[i] & np.isfinite(S[i]).astype(s.aperture.dtype), **kw)
		except Exception as e: # noqa: B902  -- the reference turns any exception into STATUS.ERROR (tessphot.py:37-49)
			r = {'status': oap.STATUS_ERROR, 'exception': repr(e)}
		if cut_override is None:
			try:
				r['thr'] = ok2p2.threshold(S[i], 0.8, full_output=True)
			except Exception: # noqa: B902
				r['thr'] = None
		out.append(r)
	return out


def compare(s, S, got, ref, check_cut=True):
	"""``got``: dict of arrays mask,status,flags,contamination,diag,cat_in_mask.  Returns stats dict."""
	n_exact = 0
	n_error_agree = 0
	n_razor = 0
	n_tie = 0
	margins = []
	dcuts = []
	for i in range(s.n_targets):
		r = ref[i]
		razor = False
		if check_cut and r.get('thr') is not None and np.isfinite(r['thr']['CUT']):
			# The threshold comes out of a Brent line search that stops at a 1e-2 relative step
			# (scipy Powell, xtol*100): last-bit differences of exp()/summation order in the KDE are
			# amplified to ~1e-8 in CUT -- numpy's own SIMD exp differs between CPUs by as much.  So CUT is
			# compared to 2e-6 relative, and mask bit-exactness is asserted whenever no pixel lies within
			# 4*|dCUT| of the oracle's CUT (the complementary test feeds the oracle's CUT to the kernel).
			thr = r['thr']
			d = got['diag'][i]
			dcut = abs(d[0] - thr['CUT'])
			assert abs(d[3] - thr['bandwidth']) <= 1e-12*abs(thr['bandwidth'])
			assert int(d[5]) == thr['nflux']
			# Two samples give a KDE with two maxima of EQUAL height: which one the first argmax of the FFT density lands on is
			# decided by the transform's rounding noise (numpy's pocketfft there, a radix-2 FFT here) -- seen once in 5 936 fuzz
			# targets, a sum image with two positive pixels.  The threshold is then not comparable; the outputs below still are.
			tie = thr.get('nflux_cut', 3) <= 2 and dcut > 2e-6*max(1.0, abs(thr['CUT']))
			if tie:
				n_tie += 1
			else:
				# the KDE's argmax (the start of the Powell search): the same grid point.  (The search is forgiving -- a start one grid
				# step off usually ends in the same mode -- which hid a linear binning that went wrong above 512 samples until round 6.)
				assert abs(d[4] - thr['max_guess']) <= 1e-9*max(1.0, abs(thr['max_guess'])), f"target {i}: KDE argmax {d[4]} vs {thr['max_guess']}"
				assert dcut <= 2e-6*max(1.0, abs(thr['CUT'])), f"target {i}: CUT {d[0]} vs {thr['CUT']}"
				with np.errstate(invalid='ignore'):
					margin = np.nanmin(np.abs(S[i] - thr['CUT']))
				margins.append(margin)
				dcuts.append(dcut)
				razor = margin <= 4*dcut
		if razor:
			n_razor += 1
			continue
		assert int(got['status'][i]) == r['status'], f"target {i}: status {got['status'][i]} vs {r['status']} ({r.get('errors')}, {r.get('exception')}) flags={got['flags'][i]:#x}"
		if 'mask' in r and r['status'] != oap.STATUS_ERROR:
			np.testing.assert_array_equal(got['mask'][i].astype(bool), r['mask'], err_msg=f"target {i} mask")
			assert bool(got['flags'][i] & 1) == bool(r['using_minimum_mask']), f"target {i} min-aperture flag"
			c = r['contamination']
			if np.isnan(c):
				assert np.isnan(got['contamination'][i])
			else:
				assert abs(got['contamination'][i] - c) < 2e-6, f"target {i}: contamination {got['contamination'][i]} vs {c}"
			a, b = s.cat_offsets[i], s.cat_offsets[i+1]
			inm = np.zeros(b - a, dtype=bool)
			inm[r['target_in_mask']] = True
			np.testing.assert_array_equal(got['cat_in_mask'][a:b].astype(bool), inm)
			e = r.get('edge', {})
			fl = int(got['flags'][i])
			assert bool(fl & 2) == ('down' in e) and bool(fl & 4) == ('up' in e) and bool(fl & 8) == ('left' in e) and bool(fl & 16) == ('right' in e)
			n_exact += 1
		else:
			n_error_agree += 1   # no mask on the reference's side (ERROR): the statuses were asserted equal above
	return {'n_exact': n_exact, 'n_error_agree': n_error_agree, 'n_razor': n_razor, 'n_tie': n_tie, 'min_margin': float(np.min(margins)) if margins else np.nan,
		'max_dcut': float(np.max(dcuts)) if dcuts else 0.0}


def own_chain_check(S_dev, images, images_err, backgrounds, quality, stamp, pos_row, pos_col, tmag, starid, catalog, aperture, got_mask, got_status,
	got_flux=None, got_flux_err=None, got_flux_background=None):
	"""
	The parity chain closed at one target: the ORACLE's own sum image (its restatement of prepare.py:450-459 /
	BasePhotometry.py:1008-1019 on the same cube) -> the oracle's own mask and light curve, against the device's mask (built from
	the device's sum image).  The two sum images agree to ~1e-16 relative (float64 sums of float32 values in another order), so
	the masks can differ only where a pixel of the sum image sits within that distance (times the K2P2 threshold's sensitivity,
	see :func:`compare`) of the threshold: such a target is reported as a razor case, anything else must be equal.
	Returns ``'exact'``, ``'razor'`` or raises.
	"""
	S_or = osum.sumimage(images, quality)
	with np.errstate(invalid='ignore'):
		np.testing.assert_allclose(S_dev, S_or, rtol=1e-12, atol=0, equal_nan=True)
	try:
		ref = oap.do_photometry(S_or, images, images_err, backgrounds, stamp, pos_row, pos_col, tmag, starid, catalog, aperture)
	except Exception as e: # noqa: B902 -- any exception in the plugin is STATUS.ERROR upstream (tessphot.py:37-49)
		ref = {'status': oap.STATUS_ERROR, 'exception': repr(e)}
	same = int(got_status) == ref['status'] and (ref['status'] == oap.STATUS_ERROR or 'mask' not in ref or np.array_equal(np.asarray(got_mask).astype(bool), ref['mask']))
	if not same:
		# razor: a pixel of the sum image within the reach of the threshold's own uncertainty (2e-6 relative, see compare())
		thr = ok2p2.threshold(S_or, 0.8, full_output=True)
		with np.errstate(invalid='ignore'):
			margin = np.nanmin(np.abs(S_or - thr['CUT']))
		assert margin <= 8e-6 * max(1.0, abs(thr['CUT'])), f"masks differ off the razor's edge: margin {margin}, CUT {thr['CUT']}, status {got_status} vs {ref['status']}"
		return 'razor'
	if ref['status'] != oap.STATUS_ERROR and 'mask' in ref and got_flux is not None:
		np.testing.assert_array_equal(got_flux, ref['flux'])
		np.testing.assert_array_equal(got_flux_err, ref['flux_err'])
		if got_flux_background is not None and backgrounds is not None:
			np.testing.assert_array_equal(got_flux_background, ref['flux_background'])
	return 'exact'


#--------------------------------------------------------------------------------------------------
# Edge cases of the mask builder: inputs made so that a rule of the reference that ordinary scenes never meet decides the result.
# Every case is (scene, S, cut_override or None, claim); ``claim(ref)`` asserts from the ORACLE's side alone that the case is the
# case its name says (so that a change to the simulator cannot quietly turn it into an ordinary scene).
#--------------------------------------------------------------------------------------------------
def hand_scene(H, W, targets, n_cad=2):
	"""
	A scene written by hand, cubes of zeros.  ``targets``: one dict per target with ``stars`` -- a list of
	``(row_stamp, column_stamp, tmag)``, the first one the target -- and optionally ``pos`` (the target's ``(row_stamp,
	column_stamp)`` where it is not its star's), ``tmag`` (the target's, where it is not its star's), ``target_star`` (index into
	``stars``, ``None``: the target is not in its catalogue) and ``aperture`` (``(H, W)`` int32).
	"""
	from photometry_amd import simulate
	s = simulate.Scene()
	Nt = len(targets)
	s.n_targets, s.n_cad, s.height, s.width, s.seed = Nt, n_cad, H, W, 0
	row0 = 100 + 70*np.arange(Nt)
	col0 = 144 + 70*np.arange(Nt)
	s.stamps = np.column_stack((row0, row0 + H, col0, col0 + W)).astype('int32')
	cols = {k: [] for k in ('starid', 'tmag', 'row', 'column', 'row_stamp', 'column_stamp')}
	offs = [0]
	s.target_pos_row, s.target_pos_column, s.target_tmag = np.zeros(Nt), np.zeros(Nt), np.zeros(Nt)
	s.target_starid = np.zeros(Nt, dtype='int64')
	s.aperture = np.ones((Nt, H, W), dtype='int32')
	for i, t in enumerate(targets):
		stars = t['stars']
		for j, (r, c, m) in enumerate(stars):
			cols['starid'].append(100*(i + 1) + j); cols['tmag'].append(m)
			cols['row_stamp'].append(r); cols['column_stamp'].append(c)
			cols['row'].append(r + row0[i]); cols['column'].append(c + col0[i])
		offs.append(offs[-1] + len(stars))
		ts = t.get('target_star', 0)
		s.target_starid[i] = 100*(i + 1) + (99 if ts is None else ts)
		pos = t['pos'] if 'pos' in t else stars[ts][:2]
		s.target_pos_row[i], s.target_pos_column[i] = pos[0] + row0[i], pos[1] + col0[i]
		s.target_tmag[i] = t['tmag'] if 'tmag' in t else stars[ts][2]
		if 'aperture' in t:
			s.aperture[i] = t['aperture']
	s.cat_offsets = np.asarray(offs, dtype='int64')
	s.catalog = {k: np.asarray(v, dtype='int64' if k == 'starid' else 'float32') for k, v in cols.items()}
	s.time = 1325.0 + np.arange(n_cad)*1800.0/86400.0
	s.timecorr = np.zeros(n_cad)
	s.quality = np.zeros(n_cad, dtype='int32')
	s.cadence_s = 1800.0
	s.jitter = np.zeros((n_cad, 2))
	s.images = np.zeros((Nt, H, W, n_cad), dtype='float32')
	s.images_err = np.zeros((Nt, H, W, n_cad), dtype='float32')
	s.backgrounds = np.zeros((Nt, H, W, n_cad), dtype='float32')
	return s


def render(H, W, stars, sky=10.0, seed=1, sigma=0.9):
	"""A sum image by hand: a sky of ``sky`` +- 0.5 (seeded, so that no two pixels are equal unless the case makes them so) and
	Gaussian stars ``(row, column, height)``."""
	rng = np.random.default_rng(seed)
	S = sky + rng.uniform(-0.5, 0.5, (H, W))
	yy, xx = np.mgrid[0:H, 0:W]
	for (r, c, a) in stars:
		S = S + a*np.exp(-0.5*((yy - r)**2 + (xx - c)**2)/sigma**2)
	return S


def oracle_cuts(S):
	"""The oracle's own threshold of every sum image, 1e30 (nothing above it) where it raises or is not finite."""
	cuts = np.full(len(S), 1e30)
	for i in range(len(S)):
		try:
			c = ok2p2.threshold(S[i], 0.8)
		except Exception: # noqa: B902
			continue
		if np.isfinite(c):
			cuts[i] = c
	return cuts


def oracle_info(s, S, i, cut=None):
	"""The intermediate images of the oracle's mask builder for target ``i`` (``k2p2FixFromSum(full_output=True)``); may raise what it raises."""
	cat = s.catalog_of(i)
	c = np.column_stack((cat['column_stamp'], cat['row_stamp'], cat['tmag']))
	return ok2p2.k2p2FixFromSum(S[i], catalog=c, cut_override=cut, full_output=True, **oap.K2P2_SETTINGS)[1]


def tied_floods(info):
	"""Sizes (pixels) of the clusters whose priority flood starts from at least two markers and holds two equal values."""
	out = []
	for w in info.get('ws', []):
		inmask = w['Z'] != 0
		z = w['Z'][inmask]
		if len(set(w['markers'][inmask].tolist()) - {0}) >= 2 and len(np.unique(z)) < z.size:
			out.append(int(z.size))
	return out


def with_extra_stars(s, extra):
	"""The scene with stars ``(row_stamp, column_stamp, tmag)`` appended to the catalogues of the targets ``extra`` names (dict target -> list)."""
	cols = {k: [] for k in s.catalog}
	offs = [0]
	for i in range(s.n_targets):
		cat = s.catalog_of(i)
		add = extra.get(i, [])
		for k in cols:
			cols[k].append(cat[k])
		cols['starid'][-1] = np.concatenate((cat['starid'], s.target_starid[i] + 50 + np.arange(len(add), dtype='int64')))
		for k, v in (('row_stamp', [a[0] for a in add]), ('column_stamp', [a[1] for a in add]), ('tmag', [a[2] for a in add]),
			('row', [a[0] + s.stamps[i, 0] for a in add]), ('column', [a[1] + s.stamps[i, 2] for a in add])):
			cols[k][-1] = np.concatenate((cat[k], np.asarray(v, dtype='float32')))
		offs.append(offs[-1] + len(cols['starid'][-1]))
	s.catalog = {k: np.concatenate(v) for k, v in cols.items()}
	s.cat_offsets = np.asarray(offs, dtype='int64')
	return s


def _infos(s, S, cuts):
	"""oracle_info of every target, ``None`` where the oracle raises."""
	out = []
	for i in range(s.n_targets):
		try:
			out.append(oracle_info(s, S, i, None if cuts is None else cuts[i]))
		except Exception: # noqa: B902
			out.append(None)
	return out


def _error_is(r, text):
	assert r['status'] == oap.STATUS_ERROR and text in r.get('exception', ''), (r['status'], r.get('exception'), r.get('errors'))


#: name -> (group of the issue's list, builder); a builder returns (scene, S, cut_override or None, claim)
EDGE_CASES = {}


def _edge(name, group):
	def deco(f):
		EDGE_CASES[name] = (group, f)
		return f
	return deco


@functools.lru_cache(maxsize=None)
def edge_case(name):
	return EDGE_CASES[name][1]()


@functools.lru_cache(maxsize=None)
def edge_reference(name):
	"""The oracle's results of a case: computed once, shared by the routes that are held to it, never changed."""
	s, S, cuts, _claim = edge_case(name)
	return oracle_batch(s, S, cut_override=cuts)


def edge_cases():
	return [(name,) + tuple(edge_case(name)) for name in EDGE_CASES]


def edge_accept(name, got):
	"""The acceptance of one case for the outputs ``got`` of a route: with an override every target exact or an agreed error; without
	one the full comparison, threshold included, and nothing on the razor's edge."""
	s, S, cuts, _claim = edge_case(name)
	ref = edge_reference(name)
	if cuts is not None:
		stats = compare(s, S, got, ref, check_cut=False)
		assert stats['n_exact'] + stats['n_error_agree'] == s.n_targets, stats
	else:
		stats = compare(s, S, got, ref)
		assert stats['n_razor'] == 0 and stats['n_tie'] == 0 and stats['n_exact'] + stats['n_error_agree'] == s.n_targets, stats
	return stats


# ---- 1. plateaus: equal values inside a cluster that the watershed splits (pops by value, THEN by push age) ----
def _clipped(kind, seed):
	s, S = make_cases(kind, seed)
	for i in range(s.n_targets):
		if np.isfinite(S[i]).any():
			S[i] = np.minimum(S[i], np.nanpercentile(S[i], 90))
	return s, S, oracle_cuts(S)


def _claim_tied(min_targets=1, min_pixels=0):
	def claim(ref, s, S, cuts):
		n = sum(1 for info in _infos(s, S, cuts) if info is not None and any(z > min_pixels for z in tied_floods(info)))
		assert n >= min_targets, f"{n} targets with a flood of equal values from two markers"
	return claim


@_edge('plateau_faint15', 1)
def _plateau_faint15():
	return _clipped('faint15', 1) + (_claim_tied(3),)


@_edge('plateau_crowded', 1)
def _plateau_crowded():
	return _clipped('crowded', 3) + (_claim_tied(3),)


@_edge('plateau_wide', 1)
def _plateau_wide():
	return _clipped('wide', 8) + (_claim_tied(3),)


@_edge('plateau_huge', 1)
def _plateau_huge():
	# more than 3 072 in-mask pixels: beyond the summary words of the flood's bit set; 100 x 96: the work arrays live in HBM
	def claim(ref, s, S, cuts):
		assert not lds_resident(s.height, s.width)
		_claim_tied(1, 3072)(ref, s, S, cuts)
	return _clipped('huge', 6) + (claim,)


@_edge('plateau_crowded_62x58', 1)
def _plateau_crowded_padded():
	# the clipped crowded scene on stamps grown to 62 x 58 (rows and columns of each target's smallest value added below and to the
	# right: nothing above the threshold): the same floods on work arrays in HBM
	import copy
	s0, S0, cuts = _clipped('crowded', 3)
	H, W = 62, 58
	s = copy.copy(s0)
	s.height, s.width, s.n_cad = H, W, 2
	s.stamps = s0.stamps.copy()
	s.stamps[:, 1] = s.stamps[:, 0] + H
	s.stamps[:, 3] = s.stamps[:, 2] + W
	S = np.empty((s.n_targets, H, W))
	for i in range(s.n_targets):
		S[i] = np.nanmin(S0[i]) if np.isfinite(S0[i]).any() else np.nan
		S[i, :s0.height, :s0.width] = S0[i]
	s.aperture = np.ones((s.n_targets, H, W), dtype='int32')
	s.images = np.zeros((s.n_targets, H, W, 2), dtype='float32')
	s.images_err, s.backgrounds = s.images.copy(), s.images.copy()
	s.quality, s.time = np.zeros(2, dtype='int32'), s0.time[:2]

	def claim(ref, s, S, cuts):
		assert not lds_resident(s.height, s.width)
		_claim_tied(3)(ref, s, S, cuts)
	return s, S, cuts, claim


#: the two hand-made plateaus: the sum images (9 x 9), the two stars, and the labels the priority flood must give -- worked out by
#: hand below, in the manner of tests/test_oracle_pins.py
def _plateau_hand_images():
	A = render(9, 9, [], seed=3)
	A[1:8, 1:8] = 100.0
	A[1, 1] = 250.0      # (a spike: with the maximum above twice the plateau no column passes for saturated, k2p2v2.py:321, and both markers stay)
	B = render(9, 9, [], seed=4)
	B[1:8, 1:5] = 100.0
	B[1:8, 5:8] = 80.0   # a terrace: two levels
	B[2, 2] = 250.0
	B[6, 6] = 90.0
	return A, B


# A: the spike (1,1) pops first and labels (1,2), (2,1); from then on every value is equal and the pops come by age: marker 2 at (5,5)
# (age 0), then the two fronts ring by ring -- a pixel belongs to the marker whose front (marker 1 one pop ahead of its Manhattan
# distance, its first ring pushed before marker 2's) reaches it first.  Popping by pixel index instead lets marker 1 run along the rows.
PLATEAU_HAND_LABELS_A = np.array([
	[0, 0, 0, 0, 0, 0, 0, 0, 0],
	[0, 1, 1, 1, 1, 1, 1, 1, 0],
	[0, 1, 1, 1, 1, 2, 2, 2, 0],
	[0, 1, 1, 1, 2, 2, 2, 2, 0],
	[0, 1, 1, 2, 2, 2, 2, 2, 0],
	[0, 1, 2, 2, 2, 2, 2, 2, 0],
	[0, 1, 2, 2, 2, 2, 2, 2, 0],
	[0, 1, 2, 2, 2, 2, 2, 2, 0],
	[0, 0, 0, 0, 0, 0, 0, 0, 0]])
# B: the spike (2,2), then the whole upper level (100) from marker 1 alone: every pixel of column 4 that pops labels its neighbour in
# column 5 (level 80) before marker 2 (90, at (6,6)) pops at all.  Marker 2 then labels (5,6), (6,7), (7,6) -- (6,5) is taken.  Level 80 by
# age: the seven pixels of column 5 first (pushed during level 100), labelling (1..4,6) for marker 1; then marker 2's three, labelling
# (5,7) and (7,7); then (1..4,6), labelling (1..4,7).  Marker 2 keeps rows 5-7 of columns 6-7.
PLATEAU_HAND_LABELS_B = np.array([
	[0, 0, 0, 0, 0, 0, 0, 0, 0],
	[0, 1, 1, 1, 1, 1, 1, 1, 0],
	[0, 1, 1, 1, 1, 1, 1, 1, 0],
	[0, 1, 1, 1, 1, 1, 1, 1, 0],
	[0, 1, 1, 1, 1, 1, 1, 1, 0],
	[0, 1, 1, 1, 1, 1, 2, 2, 0],
	[0, 1, 1, 1, 1, 1, 2, 2, 0],
	[0, 1, 1, 1, 1, 1, 2, 2, 0],
	[0, 0, 0, 0, 0, 0, 0, 0, 0]])


def _plateau_hand(which):
	A, B = _plateau_hand_images()
	img, stars, expect = (A, [(1.0, 1.0, 10.0), (5.0, 5.0, 11.0)], PLATEAU_HAND_LABELS_A) if which == 'A' else (B, [(2.0, 2.0, 10.0), (6.0, 6.0, 11.0)], PLATEAU_HAND_LABELS_B)
	# two targets on the same image: each of the two stars once as the target, so both segments are compared
	s = hand_scene(9, 9, [{'stars': stars}, {'stars': stars[::-1]}])
	S = np.stack([img, img])
	cuts = np.array([50.0, 50.0])

	def claim(ref, s, S, cuts):
		info = oracle_info(s, S, 0, cuts[0])
		assert tied_floods(info) == [49]
		np.testing.assert_array_equal(info['ws'][0]['labels_ws'], expect)
		assert ref[0]['status'] == oap.STATUS_OK and ref[1]['status'] == oap.STATUS_OK
		np.testing.assert_array_equal(ref[0]['mask'], expect == 1)
		np.testing.assert_array_equal(ref[1]['mask'], expect == 2)
	return s, S, cuts, claim


@_edge('plateau_hand_flat', 1)
def _plateau_hand_flat():
	return _plateau_hand('A')


@_edge('plateau_hand_terrace', 1)
def _plateau_hand_terrace():
	return _plateau_hand('B')


@_edge('plateau_quantised', 1)
def _plateau_quantised():
	s, S = make_cases('crowded', 3)
	cuts = np.full(s.n_targets, 1e30)
	for i in range(s.n_targets):
		if not np.isfinite(S[i]).any():
			continue
		q = np.nanpercentile(np.abs(S[i]), 60)
		S[i] = np.round(S[i]/q)*q
		cuts[i] = 0.5*q      # half a step: no pixel equals it

	def claim(ref, s, S, cuts):
		for i in range(s.n_targets):
			with np.errstate(invalid='ignore'):
				assert not np.any(S[i] == cuts[i])
		_claim_tied(3)(ref, s, S, cuts)
	return s, S, cuts, claim


# ---- 2. one LDS-resident cluster of more than 2 048 pixels: all three summary words of the flood's bit set ----
@_edge('large_lds_cluster', 2)
def _large_lds_cluster():
	from photometry_amd import simulate
	s = simulate.make_scene(3, 8, 50, 50, seed=2, tmag_range=(-1.5, -0.5), max_neighbours=2, neighbour_tmag_range=(-1.5, 0.0), sigma_psf=9.0)
	simulate.fill_cubes(s, nan_fraction=0.002)
	S = osum.sumimage_batch(s.images, s.quality)

	def claim(ref, s, S, cuts):
		sizes = []
		for info in _infos(s, S, cuts):
			for w in info['ws']:
				inmask = w['Z'] != 0
				if len(set(w['markers'][inmask].tolist()) - {0}) >= 2:
					sizes.append(int(inmask.sum()))
		assert sizes and max(sizes) > 2048 and lds_resident(s.height, s.width), sizes
	return s, S, None, claim


@_edge('huge_unmarked_bump', 2)
def _huge_unmarked_bump():
	# the scanning path of the flood (more than 3 072 ranks) with a bump no catalogue star marks: the flood arrives at its foot and climbs
	# it -- pushes to ranks far BELOW the one just popped, which move the scan back
	s, S = make_cases('huge', 6)
	yy, xx = np.mgrid[0:s.height, 0:s.width]
	S[0] = S[0] + 10.0*S[0][30, 60]*np.exp(-0.5*((yy - 30)**2 + (xx - 60)**2)/3.0**2)

	def claim(ref, s, S, cuts):
		w = max(oracle_info(s, S, 0)['ws'], key=lambda w: int((w['Z'] != 0).sum()))
		inmask = w['Z'] != 0
		assert inmask.sum() > 3072 and len(set(w['markers'][inmask].tolist()) - {0}) >= 2
		# a peak of the blurred image within two pixels of the bump that no star took
		assert any(abs(r - 30) <= 2 and abs(c - 60) <= 2 and w['markers'][r, c] == 0 for r, c in w['peaks'])
	return s, S, None, claim


# ---- 3. the sample of the threshold's KDE (no override: the whole of A2 is compared) ----
def _claim_off_the_razor(ref, s, S):
	"""From the oracle alone: no pixel within 1e-3 (relative) of its threshold -- compare()'s razor escape is out of play."""
	for i in range(s.n_targets):
		thr = ref[i].get('thr')
		if thr is not None and np.isfinite(thr['CUT']):
			with np.errstate(invalid='ignore'):
				assert np.nanmin(np.abs(S[i] - thr['CUT'])) >= 1e-3*max(1.0, abs(thr['CUT'])), (i, thr['CUT'])


def _small_scene(seed, n=6):
	from photometry_amd import simulate
	s = simulate.make_scene(n, 12, 11, 11, seed=seed)
	simulate.fill_cubes(s, nan_fraction=0.0)
	return s, osum.sumimage_batch(s.images, s.quality)


@_edge('sample_cut_70000', 3)
def _sample_cut_70000():
	# a fifth of the positive pixels at or above 70 000: the flux cut of the KDE's sample (k2p2v2.py:407) bites after the trim
	s, S = _small_scene(31)
	for i in range(s.n_targets):
		S[i] = S[i]*(70000.0/np.percentile(S[i][S[i] > 0], 80))

	def claim(ref, s, S, cuts):
		for i in range(s.n_targets):
			thr = ref[i]['thr']
			assert thr['nflux_cut'] < thr['nflux'] - int(0.15*thr['nflux']), thr
		_claim_off_the_razor(ref, s, S)
	return s, S, None, claim


@_edge('sample_empty', 3)
def _sample_empty():
	# every positive pixel at or above 70 000: the sample is empty; what the oracle makes of that is the expectation
	s, S = _small_scene(32, n=3)
	S = S - np.min(S, axis=(1, 2), keepdims=True) + 70000.0
	S[2][S[2] < np.percentile(S[2], 40)] = -1.0    # ... and one with pixels that are not positive at all

	def claim(ref, s, S, cuts):
		for i in range(s.n_targets):
			assert np.all((S[i] >= 70000.0) | (S[i] <= 0)) and ref[i]['thr'] is None
		_claim_off_the_razor(ref, s, S)
	return s, S, None, claim


@_edge('sample_tiny', 3)
def _sample_tiny():
	# one, three and nine positive pixels: a sample of one has no standard deviation (NaN bandwidth, NaN threshold: nothing above it)
	s, S = _small_scene(34, n=3)
	S = -np.abs(S) - 1.0
	S[0][5, 5] = 50.0
	S[1][5, 5], S[1][5, 6], S[1][6, 5] = 50.0, 40.0, 30.0
	S[2][4:7, 4:7] = np.arange(9).reshape(3, 3)*3.0 + 20.0

	def claim(ref, s, S, cuts):
		assert [ref[i]['thr']['nflux_cut'] for i in range(3)] == [1, 3, 8] and np.isnan(ref[0]['thr']['CUT'])
		_claim_off_the_razor(ref, s, S)
	return s, S, None, claim


@_edge('sample_iqr_zero', 3)
def _sample_iqr_zero():
	# more than half of the sample one value: the interquartile range is 0, the standard deviation is not: Scott's rule takes the latter
	s, S = _small_scene(33)
	rng = np.random.default_rng(33)
	for i in range(s.n_targets):
		flat = rng.random(S[i].shape) < 0.7
		B = S[i] - np.min(S[i]) + 6.0
		S[i] = np.where(flat & (B < np.percentile(B, 85)), np.median(B), B)      # the equal values in the middle of the sample

	def claim(ref, s, S, cuts):
		from oracle.kde import select_bandwidth
		for i in range(s.n_targets):
			f = np.sort(S[i][S[i] > 0])
			f = f[:len(f) - int(0.15*len(f))]
			assert np.percentile(f, 75) == np.percentile(f, 25) and np.std(f, ddof=1) > 0
			assert abs(ref[i]['thr']['bandwidth'] - 1.059*np.std(f, ddof=1)*len(f)**-0.2) <= 1e-12*ref[i]['thr']['bandwidth']
			assert select_bandwidth(f, bw='scott', kernel='gau') == ref[i]['thr']['bandwidth']
		_claim_off_the_razor(ref, s, S)
	return s, S, None, claim


# ---- 4. geometry ----
def _blob(S, r, c, peak, h=1, w=1):
	"""A cluster painted by hand: (2h+1) x (2w+1) pixels around (r, c), falling off from ``peak`` with distinct values."""
	for dr in range(-h, h + 1):
		for dc in range(-w, w + 1):
			rr, cc = r + dr, c + dc
			if 0 <= rr < S.shape[0] and 0 <= cc < S.shape[1]:
				S[rr, cc] = peak/(1.0 + 0.5*(dr*dr + dc*dc) + 0.013*dr + 0.007*dc)
	return S


@_edge('geometry_one_row', 4)
def _geometry_one_row():
	S = render(1, 12, [(0, 6, 300.0)], seed=41)[None]
	s = hand_scene(1, 12, [{'stars': [(0.0, 6.0, 10.0)]}])

	def claim(ref, s, S, cuts):
		assert np.sum(S[0] > cuts[0]) >= 3 and ref[0]['status'] == oap.STATUS_WARNING and ref[0]['using_minimum_mask']
	return s, S, np.array([50.0]), claim


@_edge('geometry_one_column', 4)
def _geometry_one_column():
	S = render(12, 1, [(6, 0, 300.0)], seed=42)[None]
	s = hand_scene(12, 1, [{'stars': [(6.0, 0.0, 10.0)]}])

	def claim(ref, s, S, cuts):
		assert np.sum(S[0] > cuts[0]) >= 3 and ref[0]['status'] == oap.STATUS_WARNING and ref[0]['using_minimum_mask']
	return s, S, np.array([50.0]), claim


@_edge('geometry_bleed_column', 4)
def _geometry_bleed_column():
	# A bleed column on a stamp of more than 256 pixels.  DBSCAN's core rule (four pixels above the threshold in the 3 x 3 neighbourhood)
	# cannot be met by a cluster ONE pixel wide: two columns is the narrowest window a cluster of the reference has.
	S = render(17, 17, [(13, 3, 200.0)], seed=43)
	for r in range(2, 15):
		S[r, 8] = 1000.0*(1 + 0.001*np.sin(r))
		S[r, 9] = 400.0 + r
	s = hand_scene(17, 17, [{'stars': [(8.0, 8.4, 5.0), (13.0, 3.0, 10.0)]}])

	def claim(ref, s, S, cuts):
		info = oracle_info(s, S, 0, cuts[0])
		cols = np.flatnonzero(np.any(info['labels_ini'] == info['labels_ini'][8, 8], axis=0))
		assert list(cols) == [8, 9] and ref[0]['status'] == oap.STATUS_OK and ref[0]['mask'][8, 8]
	return s, S[None], np.array([50.0]), claim


def _strip(H, W):
	# a stamp five pixels across that straddles the 64 rows / columns of the bit-row labelling: one cluster touching the LAST column
	# (row), the target's, and one in the middle
	S = render(H, W, [], seed=44 + H + W)
	if W > H:
		_blob(S, 2, W - 2, 400.0); _blob(S, 2, W//2, 300.0)
		stars = [(2.0, W - 2.0, 10.0), (2.0, float(W//2), 11.0)]
	else:
		_blob(S, H - 2, 2, 400.0); _blob(S, H//2, 2, 300.0)
		stars = [(H - 2.0, 2.0, 10.0), (float(H//2), 2.0, 11.0)]
	s = hand_scene(H, W, [{'stars': stars}, {'stars': stars[::-1]}])

	def claim(ref, s, S, cuts):
		m = ref[0]['mask']
		assert ref[0]['status'] == oap.STATUS_OK and (np.any(m[:, -1]) if W > H else np.any(m[-1, :])) and ref[1]['status'] == oap.STATUS_OK
	return s, np.stack([S, S]), np.array([50.0, 50.0]), claim


for _H, _W in ((5, 64), (5, 65), (64, 5), (65, 5)):
	_edge(f'geometry_strip_{_H}x{_W}', 4)(functools.partial(_strip, _H, _W))


@_edge('geometry_target_pixel', 4)
def _geometry_target_pixel():
	# where the target's pixel comes from (photometry.py:107): Python's round -- half to even -- and Python's indexing: -1 is the last row
	# (column), and an index past that raises.  12 x 12; a cluster on the last row, one on the last column, one of 3 x 3 pixels in the middle.
	S = render(12, 12, [], seed=45)
	_blob(S, 11, 5, 400.0); _blob(S, 5, 11, 350.0); _blob(S, 5, 5, 300.0)
	stars = [(11.0, 5.0, 10.0), (5.0, 11.0, 10.5), (5.0, 5.0, 11.0)]
	targets = [
		{'stars': stars, 'pos': (-0.6, 5.0)},                                          # row -1: the last row's cluster
		{'stars': [stars[1], stars[0], stars[2]], 'pos': (5.0, -1.4)},                 # column -1: the last column's
		{'stars': [stars[2], stars[0], stars[1]], 'pos': (3.5, 5.0)},                  # 3.5 -> 4: inside the middle cluster (rows 4-6)
		{'stars': [stars[2], stars[0], stars[1]], 'pos': (6.5, 5.0)},                  # 6.5 -> 6: inside
		{'stars': [stars[2], stars[0], stars[1]], 'pos': (2.5, 5.0)},                  # 2.5 -> 2: outside it: minimum aperture
		{'stars': [stars[2], stars[0], stars[1]], 'pos': (7.5, 5.0)},                  # 7.5 -> 8: outside
		{'stars': stars, 'pos': (-12.6, 5.0)},                                         # row -13: IndexError
		{'stars': stars, 'pos': (5.0, 12.4)},                                          # column 12: IndexError
		{'stars': stars, 'pos': (12.4, 5.0)},                                          # row 12: IndexError
		{'stars': stars, 'pos': (5.0, -12.6)},                                         # column -13: IndexError
	]
	s = hand_scene(12, 12, targets)

	def claim(ref, s, S, cuts):
		assert ref[0]['status'] == oap.STATUS_OK and ref[0]['mask'][11, 5] and not ref[0]['using_minimum_mask']
		assert ref[1]['status'] == oap.STATUS_OK and ref[1]['mask'][5, 11] and not ref[1]['using_minimum_mask']
		for i in (2, 3):
			assert not ref[i]['using_minimum_mask'] and ref[i]['mask'][5, 5] and np.flatnonzero(np.any(ref[i]['mask'], axis=1)).tolist() == [4, 5, 6]
		for i in (4, 5):
			assert ref[i]['using_minimum_mask']
		for i in (6, 7, 8, 9):
			_error_is(ref[i], 'IndexError')
	return s, np.stack([S]*len(targets)), np.full(len(targets), 50.0), claim


# ---- 5. the catalogue ----
def _three_peaks(h_left, h_right):
	"""17 x 17: ONE cluster with three peaks -- (8,5) and (8,11), mirror images of each other about column 8 (bit for bit: the sum of
	the two is formed first), and (13,8) -- on a sky below the threshold."""
	yy, xx = np.mgrid[0:17, 0:17]
	g = lambda r, c, a: a*np.exp(-0.5*((yy - r)**2 + (xx - c)**2)/1.6**2) # noqa: E731
	G = (g(8, 5, h_left) + g(8, 11, h_right)) + g(13, 8, 250.0)
	return np.where(G > 60.0, G, render(17, 17, [], seed=51))


@_edge('catalogue_star_to_peak', 5)
def _catalogue_star_to_peak():
	# how a star finds its peak (k2p2v2.py:144-153): np.argmin's rules -- NaN counts as the minimum, the first of equal distances wins
	# (the peaks come sorted by intensity, equal ones in raster order) -- and the strict limits 2 sqrt 2 / 5 sqrt 2 around Tmag 7
	Seq, Sne = _three_peaks(300.0, 300.0), _three_peaks(280.0, 300.0)
	one = render(17, 17, [], seed=52)
	_blob(one, 5, 5, 400.0); _blob(one, 13, 13, 300.0)     # two clusters of one peak each: (5,5) and (13,13)
	low = (13.0, 8.0, 9.0)
	targets = [
		({'stars': [low, (8.0, 8.0, 6.0)]}, Seq),                       # 0: midway between equal peaks: the first in raster order, (8,5)
		({'stars': [low, (8.0, 8.0, 6.0)]}, Sne),                       # 1: midway between unequal peaks: the brighter, (8,11)
		({'stars': [(5.0, 5.0, 9.0), (np.nan, 13.0, 9.0)]}, one),       # 2: NaN row_stamp
		({'stars': [(5.0, 5.0, 9.0), (13.0, np.nan, 9.0)]}, one),       # 3: NaN column_stamp
		({'stars': [(7.0, 7.0, 7.5)], 'pos': (5.0, 5.0)}, one),         # 4: exactly 2 sqrt 2 from (5,5), fainter than 7: no match
		({'stars': [(10.0, 10.0, 6.5)], 'pos': (5.0, 5.0)}, one),       # 5: exactly 5 sqrt 2 from (5,5), brighter than 7: no match ((13,13) is nearer: 3 sqrt 2)
		({'stars': [(8.0, 8.0, 7.0)], 'pos': (5.0, 5.0)}, one),         # 6: Tmag exactly 7.0 is not fainter than 7: 3 sqrt 2 is within 5 sqrt 2
		({'stars': [(8.0, 8.0, 7.5)], 'pos': (5.0, 5.0)}, one),         # 7: ... and the same star a little fainter is out of reach
		({'stars': [], 'target_star': None, 'pos': (5.0, 5.0), 'tmag': 9.0}, one),   # 8: an empty catalogue on a stamp with clusters
		({'stars': [low, (np.nan, 8.0, 6.0)]}, Seq),                    # 9: a NaN position against three peaks: every distance is NaN, no match
	]
	s = hand_scene(17, 17, [t for t, _ in targets])
	S = np.stack([img for _, img in targets])

	def claim(ref, s, S, cuts):
		assert np.sqrt(8.0) == 2.0*np.sqrt(2) and np.sqrt(50.0) == 5.0*np.sqrt(2)      # the limits are met exactly
		for i, col in ((0, 5), (1, 11)):
			w = oracle_info(s, S, i, cuts[i])['ws'][0]
			assert len(w['peaks']) == 3 and w['markers'][8, col] != 0 and w['markers'][13, 8] != 0 and w['markers'].max() == 2
		w = oracle_info(s, S, 0, cuts[0])['ws'][0]
		assert w['distance'][8, 5] == w['distance'][8, 11]
		w = oracle_info(s, S, 9, cuts[9])['ws'][0]
		assert len(w['peaks']) == 3 and w['markers'].max() == 1 and w['markers'][13, 8] == 1 and ref[9]['status'] == oap.STATUS_OK
		for i in (2, 3):
			assert ref[i]['status'] == oap.STATUS_OK and ref[i]['mask'][5, 5] and len(ref[i]['target_in_mask']) == 1
		for i in (4, 7, 8):
			assert ref[i]['using_minimum_mask'] and 'No masks found' in ' '.join(ref[i]['errors']), ref[i]['errors']
		# 5: the star's nearest peak is (13,13), 3 sqrt 2 away: that cluster is kept, the target's is not
		assert ref[5]['using_minimum_mask'] and 'No mask found for main target' in ' '.join(ref[5]['errors'])
		# 6: (8,8) is 3 sqrt 2 from (5,5) AND from (13,13): the brighter peak, the target's, takes the star; the star itself lies outside the mask
		assert ref[6]['status'] == oap.STATUS_ERROR and not ref[6]['using_minimum_mask'] and ref[6]['mask'][5, 5] and ref[6]['errors'] == ['ERROR: No targets in mask.']
	return s, S, np.full(len(targets), 50.0), claim


@_edge('catalogue_overflow', 5)
def _catalogue_overflow():
	# the overflow rule (k2p2v2.py:579-623) with a star OUTSIDE the stamp and a star of NaN Tmag inside the mask in the catalogue
	s, S = make_cases('bright', 4)
	extra = {}
	for i in range(s.n_targets):
		extra[i] = [(-4.0, 3.0, 9.0), (3.0, s.width + 2.5, 9.0), (s.height + 2.0, 3.0, 9.0), (3.0, -3.0, 9.0), (float(round(s.star_params[i, 0, 0])), float(round(s.star_params[i, 0, 1])), np.nan)]
	s = with_extra_stars(s, extra)
	for i in range(0, s.n_targets, 3):
		# a pixel of the bleed column that was never observed: the hole is filled (k2p2v2.py:549-554) and the overflow rule's medians meet a NaN
		S[i, int(round(s.star_params[i, 0, 0])) + 1, int(round(s.star_params[i, 0, 1]))] = np.nan
	cuts = oracle_cuts(S)

	def claim(ref, s, S, cuts):
		n = 0
		for i in range(s.n_targets):
			cat = s.catalog_of(i)
			c = np.column_stack((cat['column_stamp'], cat['row_stamp'], cat['tmag']))
			try:
				with_rule = ok2p2.k2p2FixFromSum(S[i], catalog=c, cut_override=cuts[i], **oap.K2P2_SETTINGS)[0]
				without = ok2p2.k2p2FixFromSum(S[i], catalog=c, cut_override=cuts[i], **dict(oap.K2P2_SETTINGS, extend_overflow=False))[0]
			except Exception: # noqa: B902
				continue
			if with_rule is not None and not np.array_equal(with_rule, without):
				n += 1
				nan_star = len(cat['starid']) - 1
				assert 'mask' not in ref[i] or nan_star not in ref[i]['target_in_mask'] or np.isnan(cat['tmag'][nan_star])
		assert n >= 3, n
		assert sum(1 for i in range(s.n_targets) if 'mask' in ref[i] and (len(s.catalog_of(i)['starid']) - 1) in ref[i]['target_in_mask']) >= 3
	return s, S, cuts, claim


@_edge('catalogue_contamination', 5)
def _catalogue_contamination():
	S = render(12, 12, [], seed=53)
	_blob(S, 5, 5, 400.0)
	ap = np.ones((12, 12), dtype='int32')
	ap[9, 8] = 32      # not collected: bit 0 (value 1, "pixel collected") cleared on one of the nine pixels of the minimum aperture around (9, 9)
	targets = [
		# the only star in the mask is not the target and is fainter: 1 - 10^(0.4 (12 - 10)) < 0 is clamped to 0
		{'stars': [(5.0, 5.0, 12.0)], 'target_star': None, 'pos': (5.0, 5.0), 'tmag': 10.0},
		# minimum aperture with a pixel that was not collected
		{'stars': [(9.0, 9.0, 10.0), (5.0, 5.0, 11.0)], 'aperture': ap},
	]
	s = hand_scene(12, 12, targets)

	def claim(ref, s, S, cuts):
		assert ref[0]['status'] == oap.STATUS_OK and ref[0]['contamination'] == 0 and ref[0]['skip_targets'] == [100]
		assert ref[1]['using_minimum_mask'] and int(ref[1]['mask'].sum()) == 8 and not ref[1]['mask'][9, 8]
	return s, np.stack([S, S]), np.array([50.0, 50.0]), claim


# ---- 6. errors and signs ----
@_edge('error_no_peaks', 6)
def _error_no_peaks():
	# a constant image above the threshold: one cluster, its blurred image is constant, peak_local_max calls that trivial: no peak, and
	# np.argmin of the empty distance array raises (k2p2v2.py:146)
	s = hand_scene(9, 9, [{'stars': [(4.0, 4.0, 10.0)]}])
	return s, np.full((1, 9, 9), 5.0), np.array([1.0]), lambda ref, s, S, cuts: _error_is(ref[0], 'ValueError')


@_edge('negative_cut', 6)
def _negative_cut():
	# a background-subtracted sum image below zero and a threshold of -5: two clusters on a stamp of more than 256 pixels whose fluxes
	# above the threshold are partly negative, and so is the minimum of their blurred images.  (The peak threshold of
	# peak_local_max is max(min, ws_thres * max) with ws_thres = 0: never below zero, whatever the signs.)  The second target's other
	# star is out of every peak's reach.
	S = render(17, 17, [(5, 5, 14.0), (12, 11, 13.0)], sky=-10.0, seed=61, sigma=1.3)
	targets = [
		{'stars': [(5.0, 5.0, 10.0), (12.0, 11.0, 10.5)]},
		{'stars': [(12.0, 11.0, 10.5), (1.0, 15.0, 12.0)]},
	]
	s = hand_scene(17, 17, targets)
	cuts = np.array([-5.0, -5.0])

	def claim(ref, s, S, cuts):
		for i in (0, 1):
			info = oracle_info(s, S, i, cuts[i])
			assert len(info['ws']) == 2 and all(w['distance'].min() < 0 and np.any(w['Z'] < 0) for w in info['ws'])
			assert ref[i]['status'] == oap.STATUS_OK and not ref[i]['using_minimum_mask']
	return s, np.stack([S, S]), cuts, claim


@_edge('marker_off_the_mask', 6)
def _marker_off_the_mask():
	# A peak of the blurred image on a pixel that is NOT in the cluster's core: a hole (below the threshold, so Z = 0 there) inside a ring of
	# positive pixels, on a plain of negative fluxes above a negative threshold -- the ring's own pixels are pulled down by the plain
	# around them, the hole is not.  The star on the hole takes that peak; ndimage.label numbers it 1 (first in raster order); markers *
	# mask drops it: the flood's labels are {0, 2}, a GAP, and k2p2v2.py:230-242 -- which counts the labels -- keeps nothing of the
	# cluster (targets 0, 1).  With that star alone no marker survives at all (target 2).
	rng = np.random.default_rng(62)
	S = np.full((11, 11), -300.0)
	S[1:10, 1:10] = -100.0 + rng.uniform(-1, 1, (9, 9))
	S[2:5, 2:5] = 10.0 + rng.uniform(-0.1, 0.1, (3, 3))
	S[3, 3] = -300.0
	S[7, 7] = 500.0
	hole, peak = (3.0, 3.0, 10.0), (7.0, 7.0, 10.5)
	s = hand_scene(11, 11, [{'stars': [hole, peak]}, {'stars': [peak, hole]}, {'stars': [hole]}])
	cuts = np.full(3, -200.0)

	def claim(ref, s, S, cuts):
		for i in (0, 1, 2):
			w, = oracle_info(s, S, i, cuts[i])['ws']
			assert w['Z'][3, 3] == 0 and [3, 3] in w['peaks'].tolist() and w['markers'][3, 3] == 1       # the marker on Z == 0
			labels = sorted(set(w['labels_ws'].ravel().tolist()))
			assert labels == ([0, 2] if i < 2 else [0]), labels                                            # the gap / no marker left
			assert ref[i]['status'] == oap.STATUS_WARNING and ref[i]['using_minimum_mask'] and 'No masks found' in ' '.join(ref[i]['errors'])
	return s, np.stack([S]*3), cuts, claim
