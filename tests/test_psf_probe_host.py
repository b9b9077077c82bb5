# -*- coding: utf-8 -*-
"""
The premises of the walk-free probe of ``tp_psf_fit`` (``tests/psf_probe_common.py``) and the conditions on its inputs, on the CPU:
what a Nelder-Mead walk does on a constant objective, that a NaN background or a NaN variance floor makes the objective constant,
that the "store wraps" points ask for more sets than the kernel keeps, that the on-knot points are on their knots, and the floor the
device test's bound is derived from -- the oracle's two forms of the pixel integral against each other on every probe point.

Measured here (relative to the peak): the two forms differ by at most 1.3e-15 over the probe points (``FLOOR`` = 2e-15).  The
biquartic form of the cached path, restated in numpy below, departs from FITPACK by 9.2e-15 on every point -- the grid step it scales
with, ``h = t[5] - t[4]``, is a difference of two knots near -6.2 and carries their rounding (4e-15 relative, twice in ``h * h``) --
well inside the ``100 x FLOOR`` = 2e-13 the device is allowed, so both paths share the one bound.
"""
import numpy as np
import pytest
import psf_err_common as pe
import psf_probe_common as pc


# ---- the walk ----
@pytest.mark.parametrize('x0', [pc.wrap_stars(S).ravel() for S in range(1, 6)] + [np.array([5.2, 0.0, 30000.0, 0.0, 4.7, 9000.0]),
	np.array([2e6, 3.0, 9000.0])], ids=['1', '2', '3', '4', '5', 'zeros', 'far'])
def test_constant_objective_walk(x0):
	"""scipy's Nelder-Mead and the oracle's restatement on a constant objective: the same iteration count, ``success``, and the start
	point back bit for bit -- also as the second cadence of a chain (``maxiter`` 500)."""
	from scipy.optimize import minimize
	for maxiter in (1500, 500):
		res = minimize(lambda p: 0.0, x0, method='Nelder-Mead', options={'maxiter': maxiter})
		x, success, nit = pc.constant_walk(x0, maxiter)
		assert res.success and success and res.nit == nit and 1 < nit < 100
		assert np.asarray(res.x).tobytes() == x0.tobytes() and x.tobytes() == x0.tobytes()
	print(len(x0) // 3, 'stars:', nit, 'iterations')


def test_walk_of_a_vector_with_zeros():
	"""A zero parameter steps to 0.00025 (scipy's ``zdelt``), every other one by 5 %; the walk is shorter (the simplex starts smaller)."""
	x0 = np.array([0.0, 0.0, 30000.0])
	points = []
	x, success, nit = pc.constant_walk(x0, record=points)
	assert success and x.tobytes() == x0.tobytes()
	np.testing.assert_array_equal(points[:4], [x0, [0.00025, 0.0, 30000.0], [0.0, 0.00025, 30000.0], [0.0, 0.0, 1.05 * 30000.0]])
	# the count follows the largest step alone: 5 % of 30 000 halves 24 times to 1e-4, 5 % of 5 twelve times, 0.00025 twice
	assert nit == 25 and pc.constant_walk(np.array([5.0, 0.0, 0.0]))[2] == 13 and pc.constant_walk(np.zeros(3))[2] == 3


# ---- the objective ----
def test_objective_is_exactly_zero():
	"""``lhood`` with a NaN background under a finite image, and with a NaN variance floor: exactly 0.0 at any point."""
	from oracle.psf_photometry import lhood
	psf = pe.oracle_psf('spoc', (1000, 1011, 800, 811))
	rng = np.random.default_rng(3)
	img = rng.normal(100.0, 10.0, (11, 11)).astype('float32')
	for x in (pc.wrap_stars(3).ravel(), np.array([5.2, 4.7, 30000.0])):
		v = lhood(x, psf, img, np.full((11, 11), np.nan, dtype='float32'))
		assert v == 0.0 and not np.signbit(v)
		v = lhood(x, psf, img, np.zeros((11, 11), dtype='float32'), readnoise=np.nan)
		assert v == 0.0 and not np.signbit(v)
		assert lhood(x, psf, img, np.zeros((11, 11), dtype='float32')) > 0


# ---- conditions on the inputs ----
def test_store_wraps_points_ask_for_more_sets_than_are_kept():
	counts = []
	for S in range(1, 6):
		(probe,) = pc.probe_points()[f'inst_spoc_{S}']
		assert len(probe.fitted) == S
		keys = pc.walk_keys(probe.x0)
		assert {k[0] for k in keys} == set(range(S))
		counts.append(len(keys))
		if S >= 2:
			assert len(keys) > pc.STORE_SLOTS, (S, len(keys))           # the store wraps: a set built early is gone when the walk is over
		else:
			assert len(keys) > pc.ONE_STAR_POOL, len(keys)              # more than the one-star pool caches
		per_star = [sum(1 for k in keys if k[0] == s) for s in range(S)]
		assert min(per_star) > (pc.ONE_STAR_POOL if S == 1 else 1), per_star     # every star outgrows its share of the pool
	print('distinct (star, column interval, row interval) keys of the walk, 1 .. 5 stars:', counts)
	assert pc.STORE_SLOTS == 16 and pc.ONE_STAR_POOL == 2
	# two stars whose whole walk stays in one and the same pair of intervals
	(probe,) = pc.probe_points()['same_intervals']
	keys = sorted(pc.walk_keys(probe.x0))
	assert len(keys) == 2 and keys[0][1:] == keys[1][1:] and [k[0] for k in keys] == [0, 1], keys


def test_probe_points_are_what_they_claim():
	P = pc.probe_points()
	model = pe.host_model('spoc')
	# the sweep visits the nine intervals of both axes
	ky = {pc.phase_interval(model.ty, p.x0[0, 0])[0] for p in P['phase_sweep']}
	kx = {pc.phase_interval(model.tx, p.x0[0, 1])[0] for p in P['phase_sweep']}
	assert len(ky) == 9 and len(kx) == 9 and len(P['phase_sweep']) == 17
	# on a knot: a phase of exactly 0; the last two one rounding beside it
	for p in P['phase_knots'][:10]:
		assert pc.phase_interval(model.ty, p.x0[0, 0])[1] == 0.0 and pc.phase_interval(model.tx, p.x0[0, 1])[1] == 0.0
	for p in P['phase_knots'][10:]:
		for ph in (pc.phase_interval(model.ty, p.x0[0, 0])[1], pc.phase_interval(model.tx, p.x0[0, 1])[1]):
			assert 0.0 < min(ph, 1.0 - ph) < 1e-14
	halves = sorted({float(v) for p in P['phase_knots'] for v in p.x0[0, :2] if v % 1.0 == 0.5})
	assert halves == [3.5, 4.5, 5.5, 6.5] and [np.rint(v) for v in halves] == [4.0, 4.0, 6.0, 6.0]
	assert any(v < 0 for p in P['phase_knots'] for v in p.x0[0, :2])
	# distance exactly 5 at the offsets (3, 4) and (5, 0) of the integer position; nothing inside the disc of the star 5.1 px outside
	(p,) = P['cutoff_integer']
	ii, jj = np.mgrid[0:11, 0:11]
	d = np.sqrt((jj - p.x0[0, 1])**2 + (ii - p.x0[0, 0])**2)
	assert d[8, 9] == 5.0 and d[9, 8] == 5.0 and d[10, 5] == 5.0 and d[5, 0] == 5.0 and np.sum(d == 5.0) == 12
	for p in P['outside_5p1']:
		assert np.all(pc.expected_pixels(p) == 0.0)
	(p,) = P['outside_4p9']
	alone = pe.oracle_psf('spoc', p.stamp).integrate_to_image(p.x0[1:2].copy(), cutoff_radius=5)
	assert np.count_nonzero(alone) == 1 and alone[4, 10] > 0
	# the trimmed corners: phases +-0.499 at the largest radius the cached path takes
	for p in P['cutoff_5p25']:
		assert p.cutoff == 5.25 and np.all(np.abs(np.abs(p.x0[0, :2] - np.rint(p.x0[0, :2])) - 0.499) < 1e-12)
	assert [len(p.x0) for p in P['mixed']] == [0, 1, 3, 5, 6]
	for name, probes in P.items():
		assert sum(len(p.pixels) for p in probes) <= 289, name      # a call's coefficient tables stay near 32 MB


def test_probe_inputs_layout():
	probes = pc.probe_points()['mixed']
	a = pc.probe_inputs(probes, T=2)
	n = sum(len(p.pixels) for p in probes)
	assert a['images'].shape == (n, 11, 11, 2) and not a['images'].any() and np.all(np.isnan(a['backgrounds']))
	assert np.all(a['mini'].reshape(n, -1).sum(axis=1) == 1) and a['star_offsets'][-1] == len(a['params0'])
	counts = np.diff(a['star_offsets'])
	assert sorted(set(counts)) == [0, 1, 3, 5, 6]
	t = int(np.flatnonzero(a['owner'] == 4)[3])
	np.testing.assert_array_equal(a['params0'][a['star_offsets'][t]:a['star_offsets'][t + 1]], probes[4].x0)
	assert a['mini'][t].ravel()[probes[4].pixels[3]] == 1
	assert pc.probe_inputs(probes, nan_background=False)['backgrounds'] is None


# ---- the floor of the model comparison ----
def test_floor_on_every_probe_point():
	"""The oracle's separable restatement against the literal FITPACK form on every probe point of the device test, relative to the
	peak: under ``FLOOR``, of which the device's bound is the hundredfold."""
	worst = 0.0
	for name, probes in pc.probe_points().items():
		for p in probes:
			if len(p.fitted) == 0:
				continue
			a, b, peak = pc.expected_pixels(p), pc.expected_pixels(p, 'scipy'), pc.peak_of(p)
			if peak == 0.0:
				assert not a.any() and not b.any()
				continue
			worst = max(worst, float(np.max(np.abs(a - b))) / peak)
			assert np.max(np.abs(a - b)) / peak <= pc.FLOOR, name
	print(f'the two forms of the oracle on the probe points: at most {worst:.2e} of the peak (FLOOR {pc.FLOOR:.0e})')
	assert pc.BOUND == 100 * pc.FLOOR == 2e-13


# ---- the biquartic form of the cached path, restated ----
_EDGE_POLY = np.array([
	[1 / 24, -1 / 6, 0.25, -1 / 6, 1 / 24], [0.5, -2 / 3, 0.0, 1 / 3, -0.125], [23 / 24, -1 / 6, -0.25, -1 / 6, 0.125], [1.0, 0.0, 0.0, 0.0, -1 / 24],
	[1.0, 0, 0, 0, 0], [1.0, 0, 0, 0, 0], [1.0, 0, 0, 0, 0], [1.0, 0, 0, 0, 0], [1.0, 0, 0, 0, 0],
	[23 / 24, 1 / 6, -0.25, 1 / 6, -1 / 24], [0.5, 2 / 3, 0.0, -1 / 3, 0.125], [1 / 24, 1 / 6, 0.25, 1 / 6, -0.125], [0.0, 0.0, 0.0, 0.0, 1 / 24]])


def biquartic_image(p):
	"""``poly_columns`` / ``poly_eval`` (csrc/linpsf_dev.h) and the cached path of ``model_pixel`` in numpy float64 on the oracle's
	coefficient table: per star the 25 coefficients of a pixel offset from its 13 x 13 patch, Horner in the two phases."""
	psf = pe.oracle_psf(p.kind, p.stamp)
	C, n = psf.coeffs, psf.coeffs.shape[0]
	h2 = (psf.tx[5] - psf.tx[4]) * (psf.ty[5] - psf.ty[4])
	img = np.zeros((p.H, p.W))
	for (row, col, flux) in p.fitted:
		kx, ky = pc.phase_interval(psf.tx, col), pc.phase_interval(psf.ty, row)
		if kx is None or ky is None:
			continue
		for i in range(p.H):
			for j in range(p.W):
				di, dj = i - int(np.rint(row)), j - int(np.rint(col))
				if max(abs(di), abs(dj)) > 5 or not (np.sqrt((j - col)**2 + (i - row)**2) < p.radius):
					continue
				ax, by = min(max(kx[0] + 9 * dj, 0), n - 13), min(max(ky[0] + 9 * di, 0), n - 13)
				K = h2 * (_EDGE_POLY.T @ C[ax:ax + 13, by:by + 13] @ _EDGE_POLY)
				val = 0.0
				for e in range(4, -1, -1):
					inner = K[e, 4]
					for d in range(3, -1, -1):
						inner = inner * ky[1] + K[e, d]
					val = val * kx[1] + inner
				img[i, j] += flux * val
	return img


def test_biquartic_form_stays_inside_the_bound():
	"""What the cached path's form alone costs against FITPACK: a twentieth of the bound, so the cached path needs none of its own."""
	P = pc.probe_points()
	worst = 0.0
	for name in ('inst_spoc_1', 'inst_spoc_5', 'phase_knots', 'cutoff_5p25', 'stamp_3x3'):
		for p in P[name]:
			worst = max(worst, float(np.max(np.abs(biquartic_image(p) - pc.expected_pixels(p)))) / pc.peak_of(p))
	print(f'the biquartic form restated against FITPACK: at most {worst:.2e} of the peak')
	assert worst <= pc.BOUND / 10
