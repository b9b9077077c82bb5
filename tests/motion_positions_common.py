# -*- coding: utf-8 -*-
"""
Shared inputs and the numpy restatement of ``tp_motion_interpolate`` / ``tp_motion_star_positions`` (csrc/motion.hip;
include/tessphot_hip.h states the definition): a loaded series of translation / euclidian / affine kernels applied to many
positions at many times.  tests/test_motion_positions_host.py holds the restatement to the host ``MovementKernel``,
tests/test_gpu_motion_positions.py holds the device to both.
"""
import numpy as np

MODES = ('unchanged', 'translation', 'euclidian', 'affine')
N_PARAMS = {'unchanged': 0, 'translation': 2, 'euclidian': 3, 'affine': 6}

#: jitter of the ECC modes, device or restatement against the host's np.dot: coordinates <= 4096 px (ulp 9.1e-13), four float64
#: operations of half an ulp each and cos / sin within a few ulp of 1.1e-16 times 4096 px give about 4e-12 px; np.dot may fuse
#: or reorder, so bit equality cannot be asked for; 1e-10 leaves a factor 25
JITTER_ATOL = 1e-10
#: float32 positions: share of the values that may differ by one float32 step (a cap, not a measurement: a 1e-10 px
#: disagreement in the jitter moves base + jitter across a float32 rounding boundary about 3 times in 1e5)
MAX_FLIPPED = 0.01


def kernels_of(mode, n, rng, scale=1.0):
	"""``(n, P)`` kernels of sub-pixel shifts and, for the ECC modes, a rotation of up to 1e-3 rad (2 px at the far corner)."""
	P = N_PARAMS[mode]
	if mode == 'unchanged':
		return np.empty((n, 0))
	shift = rng.normal(scale=0.4 * scale, size=(n, 2))
	if mode == 'translation':
		return shift
	theta = rng.uniform(-1e-3, 1e-3, n) * scale
	if mode == 'euclidian':
		return np.column_stack((shift, theta))
	c, s = np.cos(theta), np.sin(theta)
	k = np.column_stack((c, -s, shift[:, 0], s, c, shift[:, 1]))
	k[:, [0, 1, 3, 4]] += rng.normal(scale=2e-5 * scale, size=(n, 4))
	assert k.shape == (n, P)
	return k


def series(mode, seed=11, S=9):
	"""A series of ``S`` ascending times with two non-finite kernels: the first of the series (the first fill value is NaN) and one
	in the middle.  Returns ``(times, kernels)`` as ``load_series`` takes them."""
	rng = np.random.default_rng(seed)
	times = 1500.0 + np.cumsum(rng.uniform(0.015, 0.03, S))
	kernels = kernels_of(mode, S, rng)
	if kernels.shape[1]:
		kernels[0] = np.nan
		kernels[S // 2, -1] = np.inf
	return times, kernels


def good_of(times, kernels):
	"""The finite series and the fill kernels: ``(times[good], kernels[good], kernels[0], kernels[-1])`` (load_series' rule)."""
	good = np.isfinite(times) & np.all(np.isfinite(kernels), axis=1)
	return times[good], kernels[good], kernels[0], kernels[-1]


def query_times(times, kernels):
	"""The nodes themselves, points between nodes, points below the first and above the last good time, exactly the first and the
	last good time, and one NaN."""
	tg = good_of(times, kernels)[0]
	between = tg[:-1] + np.diff(tg) * np.array([0.5, 0.1, 0.9, 1 / 3, 0.77, 0.25, 0.6, 0.05])[:len(tg) - 1]
	return np.concatenate((times, between, [tg[0] - 0.2, tg[0] - 1e-9, tg[-1] + 1e-9, tg[-1] + 3.0], [tg[0], tg[-1]], [np.nan]))


def positions(n=40, seed=3):
	"""``n`` positions (column, row) over [0, 2100] x [0, 2050]: the four corners first, then uniform draws."""
	rng = np.random.default_rng(seed)
	xy = np.column_stack((rng.uniform(0, 2100, n), rng.uniform(0, 2050, n)))
	xy[:4] = [[0.0, 0.0], [2100.0, 0.0], [0.0, 2050.0], [2100.0, 2050.0]]
	return xy


def times33(times):
	"""33 timestamps from before the first to behind the last time of the series, two nodes among them."""
	t = np.linspace(times[0] - 0.01, times[-1] + 0.01, 33)
	t[7], t[20] = times[2], times[6]
	return np.sort(t)


# -- the restatement ------------------------------------------------------------------------------------------------------
def interpolate_ref(times, kernels, query):
	"""``tp_motion_interpolate``: ``(T, P)``.  scipy's linear interp1d (assume_sorted, bounds_error=False, fill_value=(first, last))
	over the finite series, written out: every step is one numpy operation on float64, so nothing is fused."""
	x, y, first, last = good_of(np.asarray(times, dtype='float64'), np.asarray(kernels, dtype='float64'))
	t = np.atleast_1d(np.asarray(query, dtype='float64'))
	assert len(x) >= 2
	hi = np.clip(np.searchsorted(x, t, side='left'), 1, len(x) - 1)
	lo = hi - 1
	with np.errstate(invalid='ignore'):
		slope = (y[hi] - y[lo]) / (x[hi] - x[lo])[:, None]
		out = slope * (t - x[lo])[:, None] + y[lo]
		out[t < x[0]] = first
		out[t > x[-1]] = last
	return out


def matrices_ref(mode, kern):
	"""``(T, 2, 3)``: the warp of every interpolated kernel (image_motion.py:147-177); identity + shift for a translation."""
	T = len(kern)
	M = np.tile(np.eye(2, 3), (T, 1, 1))
	if mode == 'translation':
		M[:, 0, 2], M[:, 1, 2] = kern[:, 0], kern[:, 1]
	elif mode == 'euclidian':
		c, s = np.cos(kern[:, 2]), np.sin(kern[:, 2])
		M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = c, -s, kern[:, 0]
		M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = s, c, kern[:, 1]
	elif mode == 'affine':
		M = kern.reshape(T, 2, 3).copy()
	return M


def jitter_ref(mode, M, xy, single=False):
	"""``(n, T, 2)`` float64: M [x y 1] - [x y], the products summed left to right; a translation's shift and an unchanged field's
	zero are copies.  ``single``: the product stored as float32 and the float32 position subtracted in float32 (apply_kernel's
	``np.empty_like(xy)`` for float32 positions)."""
	xy = np.asarray(xy, dtype='float64')
	n, T = len(xy), len(M)
	out = np.zeros((n, T, 2))
	if mode == 'unchanged':
		return out
	with np.errstate(invalid='ignore', over='ignore'):
		for a in range(2):
			if mode == 'translation':
				j = np.broadcast_to(M[None, :, a, 2], (n, T))
				out[:, :, a] = j.astype('float32') if single else j
				continue
			d = (M[None, :, a, 0] * xy[:, None, 0] + M[None, :, a, 1] * xy[:, None, 1]) + M[None, :, a, 2]
			if single:
				out[:, :, a] = d.astype('float32') - xy[:, None, a].astype('float32')
			else:
				out[:, :, a] = d - xy[:, None, a]
	return out


def positions_ref(base, jitter, single=False):
	"""float64(float32(base + jitter)) for float32 ``base`` (n,) and ``jitter`` (n, T): the sum in float64, or for ``single`` in float32."""
	base = np.asarray(base, dtype='float32')
	with np.errstate(invalid='ignore', over='ignore'):
		if single:
			return (base[:, None] + jitter.astype('float32')).astype('float64')
		return (base[:, None].astype('float64') + jitter).astype('float32').astype('float64')


def loaded(mode, times, kernels, **kwargs):
	from photometry_amd.motion import MovementKernel
	mk = MovementKernel(warpmode=mode, **kwargs)
	mk.load_series(times, kernels)
	return mk


def host_jitter(mk, t, xy):
	"""``(n, T, 2)``: the host ``MovementKernel.jitter`` per position."""
	import warnings
	with warnings.catch_warnings():
		warnings.simplefilter('ignore', RuntimeWarning)
		return np.stack([mk.jitter(t, float(x), float(y)) for x, y in xy])


def assert_float32_positions(got, exp):
	"""``got`` against the expected float32 positions ``exp`` (float64 arrays of float32 values): NaN where ``exp`` is, every value
	within one float32 spacing, at most MAX_FLIPPED of them different."""
	assert np.array_equal(np.isnan(got), np.isnan(exp))
	fin = ~np.isnan(exp)
	step = np.spacing(np.abs(exp[fin]).astype('float32')).astype('float64')
	assert np.all(np.abs(got[fin] - exp[fin]) <= step)
	flipped = np.mean(got[fin] != exp[fin]) if fin.any() else 0.0
	print(f"float32 positions: {flipped:.2%} of {fin.sum()} values one step apart")
	assert flipped <= MAX_FLIPPED
