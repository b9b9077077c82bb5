# -*- coding: utf-8 -*-
"""
The walk-free probe of ``tp_psf_fit`` (csrc/psfphot.hip) and the helpers the host test (``test_psf_probe_host.py``) and the device
test (``test_gpu_psf_probe.py``) share.

A cadence whose weights are all NaN (a NaN background under finite image values, or a NaN variance floor) has the objective 0 at
every point: scipy's Nelder-Mead, the oracle's restatement and the kernel accept nothing and shrink towards ``sim[0]`` -- the start
point ``x0``, kept first by the stable sort -- until the simplex is below ``xatol``.  The fit ends with ``success`` at ``x0`` bit for
bit after an iteration count that depends on ``x0`` alone, and the kernel writes ``flux = x0[2] + sum_mini (img - model(x0))``: with a
one-pixel mini aperture over ``img = 0`` that is ``f0 - model_p(x0)``, the kernel's own model of one pixel at a point the test chose,
in the instantiation under test and with whatever the walk left in the cached sets and the store.

The bound.  ``FLOOR`` is what the oracle's own two forms of the pixel integral (``PSF.integrate_to_image``, the separable restatement,
and ``integrate_to_image_scipy``, FITPACK's ``dblint``) are held to on every probe point, relative to ``peak = sum_s flux_s * max(unit
PRF of star s on the stamp)``: measured on the CPU at most 1.3e-15 over 40 random points per grid (spoc / 5, warped / 5, rect / 5,
nsub7 / none, spoc / 6.5), rounded up to one digit.  The device sums the same terms in another order, and on the cached path through
the biquartic form: it is allowed ``100 x FLOOR`` (the factor between ``psf_err_common.FORMS_RTOL`` and ``RTOL``) for
``|device - oracle| / peak + 2^-53 * f0 / peak`` -- the model's error plus the single rounding of ``f0 + (-model)`` in the output.
"""

import numpy as np
import psf_err_common as pe

MAX_STARS = pe.MAX_STARS
FLOOR = 2e-15            #: the oracle's two forms against each other, relative to the peak (test_psf_probe_host.py asserts it)
BOUND = 100 * FLOOR      #: the device against the oracle's integrate_to_image, relative to the peak
STORE_SLOTS = 16         #: kStoreSlots of psfphot.hip: the sets a target keeps in HBM
ONE_STAR_POOL = 2        #: psf_pool(1): the sets a one-star target caches in LDS
STAMP0 = (1000, 800)     #: the first row and column on the CCD of every probe stamp

_FLUXES = (30000.0, 9000.0, 14000.0, 6000.0, 11000.0, 7000.0)
_cache = {}


class Probe(object):
	"""One probe point: PRF samples ``kind``, ``cutoff`` (None: none), an ``H x W`` stamp, the listed stars ``x0`` ``(S, 3)`` = (row,
	column, flux) of which the first five are fitted, and the probed ``pixels`` (flat indices; one target each)."""

	def __init__(self, kind, cutoff, H, W, x0, pixels=None):
		self.kind, self.cutoff, self.H, self.W = kind, cutoff, int(H), int(W)
		self.x0 = np.asarray(x0, dtype='float64').reshape(-1, 3)
		self.pixels = np.arange(self.H * self.W) if pixels is None else np.asarray(pixels, dtype='int64')
		assert np.all((self.pixels >= 0) & (self.pixels < self.H * self.W))

	@property
	def stamp(self):
		return (STAMP0[0], STAMP0[0] + self.H, STAMP0[1], STAMP0[1] + self.W)

	@property
	def fitted(self):
		return self.x0[:MAX_STARS]

	@property
	def radius(self):
		return float('inf') if self.cutoff is None else float(self.cutoff)


def wrap_stars(S):
	"""``S`` stars at ``(9.02 + 0.37 s, 10.04 - 0.41 s)``: the 5 % vertices of the walk lie half a pixel away, several knot intervals."""
	return np.array([(9.02 + 0.37 * s, 10.04 - 0.41 * s, _FLUXES[s]) for s in range(S)])


def pixel_block(H, W, row, col, offsets):
	"""Flat indices of the pixels ``(rint(row) + d, rint(col) + e)`` for ``d, e`` in ``offsets`` that lie on the stamp."""
	i0, j0 = int(np.rint(row)), int(np.rint(col))
	return np.array([(i0 + d) * W + (j0 + e) for d in offsets for e in offsets if 0 <= i0 + d < H and 0 <= j0 + e < W], dtype='int64')


# --------------------------------------------------------------------------------------------------
# the oracle's side
# --------------------------------------------------------------------------------------------------
def expected_pixels(probe, form='fitpack'):
	"""The oracle's model image ``(H, W)`` of a probe point: ``PSF.integrate_to_image`` at the fitted stars (``form='scipy'``: the literal
	``integrate_to_image_scipy``)."""
	psf = pe.oracle_psf(probe.kind, probe.stamp)
	f = psf.integrate_to_image if form == 'fitpack' else psf.integrate_to_image_scipy
	return f(probe.fitted.copy(), cutoff_radius=probe.cutoff)


def peak_of(probe):
	"""``sum_s flux_s * max(unit PRF of star s)`` over the stamp: what the errors are relative to."""
	psf = pe.oracle_psf(probe.kind, probe.stamp)
	return float(sum(abs(f) * np.max(psf.integrate_to_image(np.array([[r, c, 1.0]]), cutoff_radius=probe.cutoff)) for (r, c, f) in probe.fitted))


def model_error(device_flux, probe, expect=None):
	"""The error measure ``(n_pixels,)`` of the device's ``flux`` at the probed pixels: ``|(f0 - flux) - oracle| / peak + 2^-53 f0 / peak``."""
	expect = expected_pixels(probe) if expect is None else expect
	f0, peak = probe.fitted[0, 2], peak_of(probe)
	return np.abs((f0 - np.asarray(device_flux)) - expect.ravel()[probe.pixels]) / peak + 2.0**-53 * abs(f0) / peak


def constant_walk(x0, maxiter=1500, record=None):
	"""The oracle's Nelder-Mead on the constant objective from ``x0``: ``(x, success, iterations)``; ``record``: a list that receives
	every evaluated point."""
	from oracle.psf_photometry import nelder_mead

	def objective(p):
		if record is not None:
			record.append(np.array(p, copy=True))
		return 0.0
	x, _, success, nit, _ = nelder_mead(objective, np.asarray(x0, dtype='float64').ravel(), maxiter)
	return x, bool(success), int(nit)


def phase_interval(knots, pos):
	"""The cached path's key of one axis (``axis_phase``, linpsf_dev.h, in numpy float64): the knot interval ``l - 3`` of the lower edge of
	the pixel nearest to the star, relative to the star -- the interval of the phase ``pos - rint(pos)`` in ninths of a pixel -- and
	the phase inside it.  None for a position that is never inside a cut-off."""
	kn = np.asarray(knots, dtype='float64')
	n = len(kn) - 4
	if not (abs(pos) < 1e6):
		return None
	h = kn[5] - kn[4]
	x0 = (np.rint(pos) - pos) - 0.5
	l = min(max(4 + int(np.floor((x0 - kn[4]) / h)), 4), n - 2)
	if x0 < kn[l] and l > 4:
		l -= 1
	elif x0 >= kn[l + 1] and l < n - 2:
		l += 1
	return l - 3, (x0 - kn[l]) / (kn[l + 1] - kn[l])


def walk_keys(x0, kind='spoc'):
	"""The distinct ``(star, column interval, row interval)`` keys of every point the constant-objective walk from ``x0`` evaluates (the
	first five stars): the sets the cached path has to build or fetch on its way."""
	model = pe.host_model(kind)
	points = []
	constant_walk(np.asarray(x0, dtype='float64').reshape(-1, 3)[:MAX_STARS], record=points)
	keys = set()
	for p in points:
		for s, (row, col, _) in enumerate(p.reshape(-1, 3)):
			kx, ky = phase_interval(model.tx, col), phase_interval(model.ty, row)
			if kx is not None and ky is not None:
				keys.add((s, kx[0], ky[0]))
	return keys


# --------------------------------------------------------------------------------------------------
# the device's inputs
# --------------------------------------------------------------------------------------------------
def probe_inputs(probes, T=1, nan_background=True):
	"""The host arrays of one call that holds the targets of ``probes`` (all of one stamp size; one target per probed pixel, each with the
	probe's stars): dict with float32 cubes ``images`` (zero) and ``backgrounds`` (NaN, or None with ``nan_background=False``: the caller
	passes a NaN variance floor) ``(n, H, W, T)``, ``stamps`` ``(n, 4)``, ``star_offsets`` int64 ``(n + 1,)``, ``params0``
	``(n_stars, 3)``, ``mini`` uint8 ``(n, H, W)`` with one pixel set, and ``owner`` ``(n,)``: the probe of every target."""
	H, W = probes[0].H, probes[0].W
	assert all((p.H, p.W) == (H, W) for p in probes)
	n = sum(len(p.pixels) for p in probes)
	mini = np.zeros((n, H * W), dtype='uint8')
	offs, params, owner = [0], [], np.empty(n, dtype='int64')
	t = 0
	for q, p in enumerate(probes):
		for px in p.pixels:
			mini[t, px] = 1
			owner[t] = q
			params.append(p.x0)
			offs.append(offs[-1] + len(p.x0))
			t += 1
	params0 = np.concatenate(params) if offs[-1] else np.zeros((0, 3))
	return {'images': np.zeros((n, H, W, T), dtype='float32'),
		'backgrounds': np.full((n, H, W, T), np.nan, dtype='float32') if nan_background else None,
		'stamps': np.tile(np.asarray(probes[0].stamp, dtype='int32'), (n, 1)), 'star_offsets': np.asarray(offs, dtype='int64'),
		'params0': np.ascontiguousarray(params0, dtype='float64'), 'mini': mini.reshape(n, H, W), 'owner': owner}


# --------------------------------------------------------------------------------------------------
# the probe points of test_gpu_psf_probe.py (the host test measures the floor on every one and asserts the conditions on them)
# --------------------------------------------------------------------------------------------------
def knot_position(kind, j, q, axis='x'):
	"""A position in pixel ``j`` whose lower pixel edge, seen from the star, lies exactly on a knot of the axis: the knot nearest to
	``-1 + q / 9``, ``q`` = 1 .. 8 (a phase of exactly 0 in its interval).  Only small ``j`` have such a position in float64."""
	model = pe.host_model(kind)
	kn = model.tx if axis == 'x' else model.ty
	knot = kn[np.argmin(np.abs(kn - (q / 9.0 - 1.0)))]
	pos = float(j) - (knot + 0.5)
	assert (np.rint(pos) - pos) - 0.5 == knot, (j, q)
	return pos


def probe_points():
	"""name -> list of :class:`Probe` that go into one call."""
	if 'points' in _cache:
		return _cache['points']
	P = {}
	# every instantiation: NS = 1 .. 5, cached (spoc, 5) and general (warped, 5); these are the "store wraps" points
	for kind in ('spoc', 'warped'):
		for S in range(1, 6):
			P[f'inst_{kind}_{S}'] = [Probe(kind, 5, 11, 11, wrap_stars(S))]
	# one mixed batch: 0, 1, 3, 5 and 6 listed stars (a 6 x 5 block of pixels each)
	six = np.vstack((wrap_stars(5), [(4.3, 3.6, _FLUXES[5])]))
	block = pixel_block(11, 11, 9.02, 10.04, range(-4, 2))
	P['mixed'] = [Probe('spoc', 5, 11, 11, x, block) for x in (np.zeros((0, 3)), wrap_stars(1), wrap_stars(3), wrap_stars(5), six)]
	# two stars in the same pair of knot intervals, near the origin where the 5 % steps of the walk stay inside an interval: both
	# miss at the first evaluation with equal (column, row) keys, and neither set is replaced before the read-out -- a set fetched
	# from a store slot that another star has tagged but not yet filled would stay to the end
	P['same_intervals'] = [Probe('spoc', 5, 7, 7, [(0.02, -0.03, 30000.0), (1.0, 1.0, 9000.0)])]
	# the pixel loop
	P['stamp_17x17'] = [Probe('spoc', 5, 17, 17, [(8.31, 7.74, 30000.0), (11.9, 12.2, 9000.0), (3.2, 13.6, 14000.0)])]
	P['stamp_5x23'] = [Probe('spoc', 5, 5, 23, [(2.27, 11.38, 30000.0), (1.1, 19.7, 9000.0), (3.6, 2.4, 14000.0)])]
	P['stamp_3x3'] = [Probe('spoc', 5, 3, 3, [(1.2, 0.9, 30000.0), (-2.3, 1.1, 9000.0), (4.6, 1.4, 14000.0), (1.3, -1.8, 6000.0), (0.8, 4.4, 11000.0)])]
	# phases: the nine knot intervals of a pixel in both axes (the diagonal and the anti-diagonal of the 9 x 9 pairs), 16 pixels each
	far = (-4, -1, 0, 3)
	sweep = []
	for a in range(9):
		for b in sorted({a, 8 - a}):
			row, col = 5.0 + (b - 4) / 9.0 + 0.013, 5.0 + (a - 4) / 9.0 - 0.017
			sweep.append(Probe('spoc', 5, 11, 11, [(row, col, 30000.0)], pixel_block(11, 11, row, col, far)))
	P['phase_sweep'] = sweep
	# phases exactly on a knot (pixels 0 .. 3: a knot is no float64 position further in; two of them negative), the half pixels
	# (rint ties to even: 4.5 -> 4, 5.5 -> 6, 3.5 -> 4, 6.5 -> 6), and positions one rounding away from a knot
	def on(j, q, axis):
		return knot_position('spoc', j, q, axis)
	kn = pe.host_model('spoc').tx
	knots = []
	for (row, col) in ((on(0, 3, 'y'), on(1, 4, 'x')), (on(1, 7, 'y'), on(0, 6, 'x')), (on(2, 5, 'y'), on(3, 1, 'x')), (on(0, 8, 'y'), on(2, 1, 'x')),
			(4.5, 5.5), (5.5, 4.5), (3.5, 6.5), (6.5, 3.5), (on(1, 5, 'y'), 5.5), (4.5, on(2, 5, 'x')),
			(5.0 - (kn[52] + 0.5), 6.0 - (kn[55] + 0.5)), (6.0 - (kn[54] + 0.5), 5.0 - (kn[50] + 0.5))):
		knots.append(Probe('spoc', 5, 11, 11, [(row, col, 30000.0)], pixel_block(11, 11, row, col, far)))
	P['phase_knots'] = knots
	# a star 4.9 px outside the stamp beside one inside; one 5.1 px outside alone (no pixel inside its disc); a position of 2e6
	P['outside_4p9'] = [Probe('spoc', 5, 11, 11, [(5.2, 4.7, 30000.0), (4.0, 14.9, 9000.0), (-4.9, 6.0, 14000.0)])]
	P['outside_5p1'] = [Probe('spoc', 5, 11, 11, [(4.0, 15.1, 30000.0)]), Probe('spoc', 5, 11, 11, [(-5.1, 6.0, 30000.0)], np.arange(0, 121, 7))]
	P['invalid_star'] = [Probe('spoc', 5, 11, 11, [(5.2, 4.7, 30000.0), (2e6, 3.0, 9000.0), (4.0, -2e6, 14000.0)])]
	P['invalid_star_general'] = [Probe('warped', 5, 11, 11, [(5.2, 4.7, 30000.0), (2e6, 3.0, 9000.0), (4.0, -2e6, 14000.0)])]
	# the cut-off: an integer position (offsets (3, 4) and (5, 0) at distance exactly 5), the trimmed corners at 5.25 and phases
	# +-0.499, the general path at 5.26 and without a cut-off on the same grid
	P['cutoff_integer'] = [Probe('spoc', 5, 11, 11, [(5.0, 5.0, 30000.0)])]
	corners = [(5.499, 5.499), (4.501, 4.501), (5.499, 4.501), (4.501, 5.499)]
	P['cutoff_5p25'] = [Probe('spoc', 5.25, 11, 11, [(r, c, 30000.0)], np.arange(q % 2, 121, 2)) for q, (r, c) in enumerate(corners)]
	P['cutoff_5p26'] = [Probe('spoc', 5.26, 11, 11, [(r, c, 30000.0)], np.arange(q % 2, 121, 2)) for q, (r, c) in enumerate(corners)]
	P['cutoff_none'] = [Probe('spoc', None, 11, 11, [(r, c, 30000.0)], np.arange(q % 2, 121, 2)) for q, (r, c) in enumerate(corners)]
	# the same point on the cached and on the general path
	both = [(5.31, 4.87, 30000.0), (7.6, 2.2, 9000.0)]
	P['paths_cached'] = [Probe('spoc', 5, 11, 11, both)]
	P['paths_general'] = [Probe('spoc', 5.26, 11, 11, both)]
	# other grids (tp_psf_fit_xy)
	P['grid_rect'] = [Probe('rect', 5, 11, 11, [(5.31, 4.87, 30000.0), (7.6, 2.2, 9000.0)])]
	P['grid_nsub7'] = [Probe('nsub7', None, 11, 11, [(5.31, 4.87, 30000.0), (7.6, 2.2, 9000.0)])]
	P['grid_coarse'] = [Probe('coarse', 5, 11, 11, [(5.31, 4.87, 30000.0), (7.6, 2.2, 9000.0)])]
	# layouts
	P['layout'] = [Probe('spoc', 5, 11, 11, [(5.31, 4.87, 30000.0), (7.6, 2.2, 9000.0)], np.arange(0, 121, 3))]
	_cache['points'] = P
	return P


def reference(name):
	"""Per probe of a call, computed once per process: ``(expected image, peak, iterations of the constant walk)``."""
	key = ('reference', name)
	if key not in _cache:
		out = []
		for p in probe_points()[name]:
			if len(p.fitted) == 0:
				out.append((np.zeros((p.H, p.W)), 0.0, 0))
				continue
			x, success, nit = constant_walk(p.fitted)
			assert success and x.tobytes() == p.fitted.tobytes()
			out.append((expected_pixels(p), peak_of(p), nit))
		_cache[key] = out
	return _cache[key]
