# -*- coding: utf-8 -*-
"""
Light-curve diagnostics (``tp_lightcurve_diagnostics``, csrc/diagnostics.hip) at the edges of its hand-written logic: the case
builders shared by tests/test_gpu_diagnostics_edges.py (kernel against the oracle) and tests/test_oracle_diagnostics_edges.py
(the oracle's own known answers on the same inputs), and the launch / comparison helpers of tests/test_gpu_diagnostics.py.

Every builder returns ``(time, quality, flux, flux_err, centroid, kwargs)`` for one launch: ``time`` ``(T,)``, ``quality`` ``(T,)``
or ``(Nt, T)``, ``flux`` / ``flux_err`` ``(Nt, T)``, ``centroid`` ``(Nt, T, 2)`` (column, row), ``kwargs`` the ``bitmask`` /
``timescale`` keywords that both ``engine.lightcurve_diagnostics`` and ``oracle.diagnostics.diagnostics`` take.  The time axis is
shared by a launch, so flux / quality / centroid variants are targets of one launch and time variants are launches of their own.
No launch here has more than 300 cadences or 32 targets (the scratch-boundary sizes are computed by :func:`lds_boundary`).

Tolerances (unchanged from tests/test_gpu_diagnostics.py): medians (mean_flux, ptp, centroid), mask_size and edge_flux are
selections / integer / the same summation order -> exact; variance, rms_hour use tree sums instead of numpy's pairwise sums ->
1e-12 relative; variability goes through a differently conditioned least-squares solve -> 1e-9 relative.
"""
import numpy as np

EXACT = ('mean_flux', 'ptp', 'pos_centroid_col', 'pos_centroid_row', 'mask_size', 'edge_flux')
DEFAULT_BITMASK = 4335 # oracle.quality.TESS_DEFAULT_BITMASK: bit 16 is not in it, bit 32 is
HOUR = 3600 / 86400


#--------------------------------------------------------------------------------------------------
def run(ctx, time, quality, flux, flux_err, cen, status=None, sumimage=None, mask=None, **kwargs):
	"""One launch through ``engine.lightcurve_diagnostics``; the ``(Nt, 10)`` block on the host."""
	from photometry_amd import engine
	Nt, T = flux.shape
	lc = engine.LightCurves(ctx, Nt, T)
	block = np.zeros((5, Nt, T))
	block[0], block[1], block[3], block[4] = flux, flux_err, cen[..., 0], cen[..., 1]
	ctx._check(ctx.lib.tp_memcpy_h2d(ctx.handle, lc.block.ptr, np.ascontiguousarray(block).ctypes.data, block.nbytes))
	out = engine.lightcurve_diagnostics(ctx, lc, ctx.array(np.asarray(time, dtype='float64')), ctx.array(np.ascontiguousarray(quality, dtype='int32')),
		status=None if status is None else ctx.array(np.asarray(status, dtype='int32')),
		sumimage=None if sumimage is None else ctx.array(np.asarray(sumimage, dtype='float64')),
		mask=None if mask is None else ctx.array(np.asarray(mask, dtype='uint8')), **kwargs)
	ctx.sync()
	return out.to_host()


def check(got, ref, tag='', variability_atol=None, skip=()):
	"""One row of the device block against the oracle's dict, column by column.  ``variability_atol``: an absolute bound on
	``variability`` instead of the relative 1e-9 (for fits that are exact or undefined, see :func:`undetrended_scale`)."""
	from photometry_amd.engine import DIAGNOSTICS_COLUMNS as COLS
	for j, key in enumerate(COLS):
		if key in skip:
			continue
		g, r = got[j], ref[key]
		if key == 'flags':
			assert int(g) == int(r), (tag, key, g, r)
		elif key in EXACT:
			assert (g == r) or (np.isnan(g) and np.isnan(r)), (tag, key, g, r)
		elif key == 'variability' and variability_atol is not None:
			assert (np.isnan(g) and np.isnan(r)) or abs(g - r) <= variability_atol, (tag, key, g, r, variability_atol)
		else:
			np.testing.assert_allclose(g, r, rtol=1e-9 if key == 'variability' else 1e-12, equal_nan=True, err_msg=f'{tag} {key}')


def oracle_rows(time, quality, flux, flux_err, cen, kwargs, sumimage=None, mask=None):
	"""``oracle.diagnostics.diagnostics`` for every target of a launch."""
	from oracle import diagnostics as odiag
	quality = np.asarray(quality)
	return [odiag.diagnostics(time, quality if quality.ndim == 1 else quality[i], flux[i], flux_err[i], cen[i],
		sumimage=None if sumimage is None else sumimage[i], mask=None if mask is None else mask[i], **kwargs) for i in range(flux.shape[0])]


def good_of(quality, i, kwargs):
	quality = np.asarray(quality)
	q = quality if quality.ndim == 1 else quality[i]
	return (q & kwargs.get('bitmask', DEFAULT_BITMASK)) == 0


def fitted_cadences(time, quality, flux, flux_err, i, kwargs):
	"""Number of cadences the cubic fit of target ``i`` sees (BasePhotometry.py:1372)."""
	good = good_of(quality, i, kwargs)
	with np.errstate(all='ignore'):
		m = np.nanmedian(flux[i][good]) if np.any(~np.isnan(flux[i][good])) else np.nan
		rel, rel_err = flux[i][good] / m - 1, np.abs(1 / m) * flux_err[i][good]
	return int(np.sum(np.isfinite(time[good]) & np.isfinite(rel) & np.isfinite(rel_err)))


def undetrended_scale(quality, flux, flux_err, i, kwargs):
	"""``nanstd(rel) / nanmedian(rel_err)`` of target ``i``: the variability with nothing subtracted.  Where the cubic is exact or
	undefined (at most 4 fitted cadences) the variability is rounding noise over a number, and the project's 1e-9 is applied
	to this scale instead of to the noise."""
	good = good_of(quality, i, kwargs)
	with np.errstate(all='ignore'):
		m = np.nanmedian(flux[i][good])
		rel, rel_err = flux[i][good] / m - 1, np.abs(1 / m) * flux_err[i][good]
		return np.nanstd(rel) / np.nanmedian(rel_err)


#--------------------------------------------------------------------------------------------------
def ordinary(rng, Nt, T):
	"""Noisy positive light curves as tests/test_gpu_diagnostics.py draws them (no NaNs): ``flux, flux_err, centroid``."""
	mean = 10**rng.uniform(2, 5, Nt)
	flux = mean[:, None] * (1 + 1e-3 * rng.standard_normal((Nt, T)) + 2e-3 * np.sin(np.arange(T) / 50.0)[None, :])
	ferr = np.sqrt(np.abs(flux)) * (1 + 0.01 * rng.standard_normal((Nt, T)))
	cen = np.stack((100.3 + 0.01 * rng.standard_normal((Nt, T)), 200.7 + 0.01 * rng.standard_normal((Nt, T))), axis=-1)
	return flux, ferr, cen


def jittered_time(rng, T):
	"""Sorted 30-minute cadences with a jitter: no sample on a bin edge."""
	return np.sort(1400.0 + np.arange(T) * (1800.0 / 86400.0) + rng.normal(0, 1e-5, T))


#: targets of :func:`selection_case`, in order
SELECTION_TARGETS = ('negative flux', 'mixed-sign centroids', 'ties at both middle ranks', 'middle ranks differ above duplicates',
	'two values', 'all equal', '+inf and -inf', 'signed zeros', '600 decades and subnormals', 'ordinary')


def selection_case(T):
	"""The radix select (block_median) on keys the seeded generator never makes: negative and mixed-sign values, ties across the
	two middle ranks, two values, one value, infinities, signed zeros, 600 decades with subnormals.  1-D quality with 7 flagged
	cadences; 'middle ranks differ above duplicates' and 'two values' drop one sample where needed so that their count is even."""
	rng = np.random.default_rng(1000 + T)
	names = SELECTION_TARGETS
	Nt = len(names)
	time = jittered_time(rng, T)
	quality = np.zeros(T, dtype='int32')
	quality[rng.choice(T, 7, replace=False)] = 32
	quality[rng.choice(T, 5, replace=False)] |= 16 # not in the default bitmask
	good = np.flatnonzero((quality & DEFAULT_BITMASK) == 0)
	n = len(good)
	flux, ferr, cen = ordinary(rng, Nt, T)
	t = {k: i for i, k in enumerate(names)}

	i = t['negative flux']
	flux[i] = -flux[i]
	i = t['mixed-sign centroids']
	cen[i] = rng.standard_normal((T, 2)) * [1.0, 1e-3]
	i = t['ties at both middle ranks'] # 101 is more than half of the samples: both middle ranks are 101
	flux[i] = rng.choice([100.0, 101.0, 102.0, 103.0], T, p=[0.15, 0.6, 0.15, 0.1])
	cen[i, :, 0] = rng.choice([7.0, 8.0, 9.0], T, p=[0.2, 0.6, 0.2])
	cen[i, :, 1] = rng.choice([-2.0, -1.0, 1.0], T, p=[0.2, 0.6, 0.2])
	i = t['middle ranks differ above duplicates'] # an even count: the lower half from {100, 101}, the upper from {103, 104, 105}
	m = n - (n % 2)
	lo = rng.choice([100.0, 101.0], m // 2, p=[0.3, 0.7]); lo[0] = 101.0
	hi = rng.choice([103.0, 104.0, 105.0], m // 2); hi[0] = 103.0
	vals = np.concatenate((lo, hi, [np.nan] * (n - m)))
	rng.shuffle(vals)
	flux[i] = rng.choice([100.0, 105.0], T) # the flagged cadences
	flux[i, good] = vals
	for c in (0, 1): # the same for the centroids, negative in the row
		vals = np.concatenate((lo, hi, [np.nan] * (n - m))) * (1.0 if c == 0 else -1.0)
		rng.shuffle(vals)
		cen[i, good, c] = vals
	i = t['two values']
	vals = np.concatenate(([5.0] * (m // 2), [7.0] * (m // 2), [np.nan] * (n - m)))
	rng.shuffle(vals)
	flux[i] = 7.0
	flux[i, good] = vals
	cen[i, :, 0] = rng.choice([-1.5, 2.5], T)
	cen[i, :, 1] = rng.choice([3.0, 3.5], T, p=[0.5, 0.5])
	i = t['all equal']
	flux[i] = 7.5
	cen[i, :, 0] = -4.25
	cen[i, :, 1] = 4.25
	i = t['+inf and -inf']
	flux[i, good[n // 3]] = np.inf
	flux[i, good[2 * n // 3]] = -np.inf
	cen[i, good[5], 0], cen[i, good[9], 0] = np.inf, -np.inf
	cen[i, good[7], 1] = -np.inf
	i = t['signed zeros'] # column: a third below, a third zeros of both signs, a third above; row: zeros of both signs only
	cen[i, :, 0] = rng.choice([-1.0, -0.0, 0.0, 1.0], T, p=[0.3, 0.2, 0.2, 0.3])
	cen[i, :, 1] = rng.choice([-0.0, 0.0], T)
	i = t['600 decades and subnormals']
	cen[i, :, 0] = 10.0**rng.uniform(-300, 300, T)
	cen[i, :, 1] = 10.0**rng.uniform(-300, 300, T) * rng.choice([-1.0, 1.0], T)
	sub = rng.choice(T, 24, replace=False)
	cen[i, sub[:12], 0] = [5e-324, 1e-323, 1e-310, 2.2e-308, 3e-320, 1e-315, 7e-309, 4e-322, 1e-312, 9e-324, 2e-317, 6e-311]
	cen[i, sub[12:], 1] = [-5e-324, 1e-323, -1e-310, 2.2e-308, -3e-320, 1e-315, -7e-309, 4e-322, -1e-312, 9e-324, -2e-317, 6e-311]
	ferr = np.sqrt(np.abs(np.where(np.isfinite(flux), flux, 100.0))) * (1 + 0.01 * rng.standard_normal((Nt, T)))
	return time, quality, flux, ferr, cen, {}


#: (cadences with quality 16, with quality 32, with quality 0) of every target of :func:`few_good_case`; all others carry 48.
#: Default bitmask: 0 and 16 are good; bitmask 16: 0 and 32 are good.
FEW_GOOD_COUNTS = ((0, 5, 0), (1, 4, 0), (2, 3, 0), (3, 2, 0), (4, 1, 0), (5, 0, 0), (1, 2, 2), (4, 3, 0))
FEW_GOOD_NAN_TARGET = 7 # its quality-16 cadences have NaN flux: all-NaN good cadences under the default bitmask only


def few_good_case(bitmask=DEFAULT_BITMASK):
	"""2-D quality (``quality_target_stride != 0``) with 0..5 good cadences per target under the default bitmask and 5..0 under
	``bitmask = 16``; the good cadences lie far apart so that a cubic through four of them is well conditioned."""
	rng = np.random.default_rng(77)
	T, Nt = 40, len(FEW_GOOD_COUNTS)
	time = jittered_time(rng, T)
	flux, ferr, cen = ordinary(rng, Nt, T)
	quality = np.full((Nt, T), 48, dtype='int32')
	for i, (n16, n32, n0) in enumerate(FEW_GOOD_COUNTS):
		# both good sets spread over the whole series: the two kinds alternate along evenly spaced slots
		slots = np.round(np.linspace(1 + (i % 3), T - 2 - (i % 2), n16 + n32 + n0)).astype(int)
		kinds = np.array([16] * n16 + [32] * n32 + [0] * n0)
		order = np.argsort(np.concatenate((np.linspace(0, 1, n16, endpoint=False), np.linspace(0.01, 1.01, n32, endpoint=False),
			np.linspace(0.02, 1.02, n0, endpoint=False))), kind='stable')
		quality[i, slots] = kinds[order]
	i = FEW_GOOD_NAN_TARGET
	flux[i, quality[i] == 16] = np.nan
	ferr[i, quality[i] == 16] = np.nan
	return time, quality, flux, ferr, cen, {'bitmask': bitmask}


def few_good_counts(bitmask):
	"""Good cadences per target of :func:`few_good_case`."""
	return [n0 + (n16 if bitmask == DEFAULT_BITMASK else n32) for (n16, n32, n0) in FEW_GOOD_COUNTS]


#--------------------------------------------------------------------------------------------------
TIME_T = 200
TIME_CASES = ('grid_dyadic', 'grid_hour', 'on_edges', 'below_edges', 'duplicate', 'nan_time', 'inf_time', 'three_stamps', 'permuted',
	'bins256', 'bins257', 'bins257_permuted')


def arange_edges(tmin, tmax, ts):
	"""The left bin edges as numpy's arange fills them: ``start + i*delta`` with ``delta = (start + step) - start``."""
	n = int(np.ceil((tmax - tmin) / ts))
	return tmin + np.arange(n) * ((tmin + ts) - tmin)


def time_case(name):
	"""Four ordinary noisy targets on a time axis the seeded generator never makes.  All cadences good but three."""
	rng = np.random.default_rng(4242)
	T, Nt = TIME_T, 4
	flux, ferr, cen = ordinary(rng, Nt, T)
	flux[1, rng.choice(T, 5, replace=False)] = np.nan
	quality = np.zeros(T, dtype='int32')
	quality[[17, 90, 151]] = 32
	grid = 1024.0 + np.arange(T) / 32.0 # exact in binary
	kwargs = {}
	if name == 'grid_dyadic': # delta = 1/16 exactly: every second sample lies on an edge
		time, kwargs = grid, {'timescale': 1 / 16}
	elif name == 'grid_hour': # delta = (1024 + 1/24) - 1024, a rounded value: edges meet samples up to that rounding
		time = grid
	elif name in ('on_edges', 'below_edges'):
		# Even cadences lie exactly on an edge tmin + i*delta, odd ones one ulp below the next, and floor((x - tmin) / delta) is off by
		# one for a part of them.  'on_edges' starts just below a power of two: the edges above it are rounded sums, and the quotient
		# of a sample on such an edge can come out below i (bin too low).  'below_edges' starts at 0: the quotient of a sample one ulp
		# below an edge rounds up to i (bin too high).
		start = 1023.9 if name == 'on_edges' else 0.0
		edges = arange_edges(start, start + (T + 2) * HOUR, HOUR)
		time = np.where(np.arange(T) % 2 == 0, edges[:T], np.nextafter(edges[1:T + 1], -np.inf))
		time[T - 1] = edges[T - 1] + 0.4 * HOUR # the end of the series inside a bin
	elif name == 'duplicate':
		time = grid.copy()
		time[60] = time[59]
		time[120:123] = time[120]
	elif name == 'nan_time':
		time = grid.copy()
		time[77] = np.nan
	elif name == 'inf_time':
		time = grid.copy()
		time[77] = np.inf
	elif name == 'three_stamps':
		time = 1024.0 + np.repeat([0.0, 0.125, 0.25], [70, 60, 70])
	elif name in ('permuted', 'bins257_permuted', 'bins256', 'bins257'):
		if name == 'permuted':
			time = grid.copy()
		else: # sorted, 200 samples in 256 (257) bins of 1/32 day: several share a bin, most bins are empty
			span = 8.0 if name == 'bins256' else 8.0 + 1 / 64
			time = np.sort(1024.0 + np.concatenate(([0.0, span], rng.uniform(0, span, T - 2))))
			kwargs = {'timescale': 1 / 32}
		if name.endswith('permuted'):
			p = rng.permutation(T)
			time, quality, flux, ferr, cen = time[p], quality[p], flux[:, p], ferr[:, p], cen[:, p]
	else:
		raise KeyError(name)
	return time, quality, flux, ferr, cen, kwargs


def n_bins(time, quality, kwargs):
	"""``len(np.arange(tmin, tmax, timescale))`` of the good cadences."""
	t = time[(quality & DEFAULT_BITMASK) == 0]
	return int(np.ceil((np.nanmax(t) - np.nanmin(t)) / kwargs.get('timescale', HOUR)))


#--------------------------------------------------------------------------------------------------
DEGENERATE_TARGETS = ('negative median', 'zero median', 'all zero', 'one inf', 'ordinary')


def degenerate_case():
	"""Fluxes for which ``rel = flux / median - 1`` is negative-scaled, infinite or NaN throughout."""
	rng = np.random.default_rng(99)
	T, Nt = 120, len(DEGENERATE_TARGETS)
	time = jittered_time(rng, T)
	quality = np.zeros(T, dtype='int32')
	quality[[3, 50, 51]] = 32
	flux, ferr, cen = ordinary(rng, Nt, T)
	flux[0] = -3.0 + 10.0 * rng.standard_normal(T)            # background-subtracted faint target: mixed signs, median < 0
	flux[1] = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0], T, p=[0.1, 0.15, 0.5, 0.15, 0.1]) # quantised: median exactly 0
	flux[2] = 0.0
	flux[3, 40] = np.inf
	ferr[:3] = 1.0 + 0.1 * rng.random((3, T))
	return time, quality, flux, ferr, cen, {}


#--------------------------------------------------------------------------------------------------
def lds_boundary(height=0, width=0):
	"""The largest ``n_cad`` whose series arrays still live in LDS, from the host formula of ``tp_lightcurve_diagnostics``
	(csrc/diagnostics.hip: ``small_bytes`` / ``series_bytes`` / ``shmem > 160 * 1024``) restated here; the next one moves to HBM."""
	threads = 256

	def shmem(n):
		tp2 = max(n, 256, 2 * (height + width))
		small = threads * 8 + (threads + 1 + 260 + 1) * 4
		series = ((tp2 + n) * 8 + 2 * n * 4 + 15) & ~15
		return small + series + 16
	n = 256
	while shmem(n + 1) <= 160 * 1024:
		n += 1
	return n


def boundary_case(T):
	"""tests/test_gpu_diagnostics.py's generator at three targets (NaNs, flagged cadences, a gap) with a 9 x 13 stamp."""
	rng = np.random.default_rng(T)
	Nt = 3
	time = jittered_time(rng, T)
	time[T // 2:] += 1.3
	quality = np.zeros(T, dtype='int32')
	quality[rng.random(T) < 0.03] = 32
	quality[rng.random(T) < 0.02] = 16
	flux, ferr, cen = ordinary(rng, Nt, T)
	flux[rng.random((Nt, T)) < 0.01] = np.nan
	ferr[np.isnan(flux)] = np.nan
	cen[rng.random((Nt, T)) < 0.01] = np.nan
	S = rng.uniform(-5, 500, (Nt, 9, 13))
	S[rng.random((Nt, 9, 13)) < 0.05] = np.nan
	mask = rng.random((Nt, 9, 13)) < 0.4
	return time, quality, flux, ferr, cen, {}, S, mask
