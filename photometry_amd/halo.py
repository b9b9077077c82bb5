# -*- coding: utf-8 -*-
"""
Halo photometry (photometry/halo/halo_photometry.py:86-265) on the device: the host layer.

Upstream the pixel weights come from the third-party ``halophot`` (``do_lc``, :179-196), which this engine does not have.  The
method implemented here is the published TV-min method (Pope et al. 2016, 2019) with the reference's settings, defined in
DESIGN.md ("Halo") and restated on the CPU in ``tests/halo_common.py``: non-negative pixel weights that sum to one
(``w = softmax(theta)``) chosen so that the total variation of the normalised light curve is minimal, by L-BFGS from uniform
weights.  Because the digits cannot be halophot's, the plugin is opt-in: ``[halo] enabled = true`` in the settings.

This module holds the host part of :99-173 (stamp size, pixel mask, split times, segments, the packing of the problems), the
batched optimiser entry :func:`tvmin` (``tp_halo_tvmin``, csrc/halo.hip), :func:`objective` (``tp_halo_objective``) and
:func:`photometry`, the whole light-curve extraction of one target that ``plugins.HaloPhotometry`` calls.
"""

import ctypes
import logging
import warnings
import numpy as np

#: the reference's settings (halo_photometry.py:86-97); only these are supported
SETTINGS = {'sub': 1, 'maxiter': 101, 'thresh': -1, 'minflux': -100.0, 'objective': 'tv', 'sigclip': False, 'random_init': False}
DIST_MAX = 20.0
#: the optimiser: history of L-BFGS, scipy's ftol / pgtol defaults as stopping rules
HISTORY, FTOL, GTOL = 10, 2.220446049250313e-09, 1e-5
#: problem states of tp_halo_tvmin
CONVERGED, CAP_REACHED, LINESEARCH_FAILED, DEGENERATE = 1, 2, 3, 4
STATUS_TEXT = {CONVERGED: 'converged', CAP_REACHED: 'iteration cap', LINESEARCH_FAILED: 'line search failed', DEGENERATE: 'degenerate'}
#: split times of the sector table (halo_photometry.py:126-133)
SECTOR_SPLITS = {1: (1339., 1347.366, 1349.315), 2: (1368.,), 3: (1395.52,), 8: (1529.50,)}
#: HALO_VER card: this engine's implementation, not halophot
VERSION = 'photometry_amd-tvmin-1'
MAX_PIXELS = 4096

logger = logging.getLogger(__name__)


def enabled(settings=None):
	"""``[halo] enabled`` of the pipeline settings (off by default)."""
	if settings is None:
		from .plugins import load_settings
		settings = load_settings()
	return settings.getboolean('halo', 'enabled', fallback=False)


def check_settings(**kwargs):
	"""Raise ``ValueError`` for any halophot setting other than the reference's values (only those are implemented)."""
	for key, value in kwargs.items():
		if key not in SETTINGS:
			raise ValueError(f"unknown Halo setting: {key}")
		if value != SETTINGS[key] and not (key == 'maxiter' and isinstance(value, (int, np.integer)) and value >= 0):
			raise ValueError(f"Halo setting {key}={value!r} is not supported (only {SETTINGS[key]!r})")


# -- host part (halo_photometry.py:99-173) ------------------------------------------------------------------------------------
def pixel_mask(aperture, cols, rows, target_row, target_column, dist_max=DIST_MAX):
	"""halo_photometry.py:118-120 on the 1-based pixel grid ``cols, rows`` of get_pixel_grid (the reference's possible one-pixel
	offset kept, see its TODO)."""
	dist = np.sqrt((cols - target_column)**2 + (rows - target_row)**2)
	return (np.asarray(aperture) & 1 != 0) & (dist <= dist_max)


def split_times(sector, time, timecorr):
	"""The split times of :125-159 (the sector table, else one gap of more than half a day between 30 % and 70 % of the
	sector), restricted to the time range; ``None`` for no split."""
	time = np.asarray(time, dtype='float64')
	good = np.isfinite(time)
	tg = time[good]
	if len(tg) == 0:
		return None
	if int(sector) in SECTOR_SPLITS:
		splits = SECTOR_SPLITS[int(sector)]
	else:
		tc = np.asarray(timecorr, dtype='float64')[good]
		t = tg - tc
		dt = np.append(np.diff(t), 0)
		t0 = np.nanmin(t)
		ttot = np.nanmax(t) - t0
		indx = (t0 + 0.30*ttot < t) & (t < t0 + 0.70*ttot) & (dt > 0.5)
		if np.sum(indx) == 1:
			i = int(np.where(indx)[0][0])
			splits = (0.5*(t[i] + t[i+1]) + tc[i],)
			logger.info("Automatically found split: %f", splits[0])
		else:
			logger.warning("No split-timestamps have been defined for this sector")
			splits = None
	if splits is not None:
		splits = tuple(s for s in splits if np.min(tg) < s < np.max(tg)) or None
	logger.debug("Split times: %s", splits)
	return splits


def segments(time, splits):
	"""Segment of every cadence (``searchsorted(split_times, time, 'right')``), -1 where the time is not finite."""
	time = np.asarray(time, dtype='float64')
	seg = np.full(len(time), -1, dtype='int64')
	good = np.isfinite(time)
	seg[good] = np.searchsorted(np.asarray(splits or (), dtype='float64'), time[good], side='right')
	return seg


class Problem(object):
	"""One segment of one target: ``pix`` (flat stamp indices), ``cad`` (cadences), ``P`` float32 (len(cad), len(pix)), ``fit``."""
	def __init__(self, pix, cad, P, fit):
		self.pix, self.cad, self.P, self.fit = pix, cad, P, fit


def build_problems(images, quality, mask, seg, minflux=SETTINGS['minflux'], bitmask=None):
	"""
	The problems of one target from its ``(rows, cols, T)`` cube: per segment, the mask pixels whose median over the segment's
	fitted cadences is not below ``minflux``, the cadences where all of them are finite, fitted where ``quality & bitmask == 0``.
	"""
	from .engine import TESS_DEFAULT_BITMASK
	bitmask = TESS_DEFAULT_BITMASK if bitmask is None else bitmask
	R, C, T = images.shape
	flat = np.asarray(images).reshape(R * C, T)
	mpix = np.flatnonzero(np.asarray(mask).ravel())
	quality = np.asarray(quality)
	out = []
	n_seg = int(seg.max()) + 1 if len(seg) and seg.max() >= 0 else 0
	for k in range(n_seg):
		c_all = np.flatnonzero(seg == k)
		fitted = c_all[(quality[c_all] & bitmask) == 0]
		with warnings.catch_warnings():
			warnings.simplefilter('ignore', RuntimeWarning)
			med = np.nanmedian(flat[np.ix_(mpix, fitted)].astype('float64'), axis=1) if len(fitted) else np.full(len(mpix), np.nan)
		pix = mpix[~(med < minflux)]
		fin = np.all(np.isfinite(flat[np.ix_(pix, c_all)]), axis=0) if len(pix) else np.ones(len(c_all), dtype=bool)
		cad = c_all[fin]
		P = np.ascontiguousarray(flat[np.ix_(pix, cad)].T, dtype='float32')
		out.append(Problem(pix, cad, P, (quality[cad] & bitmask) == 0))
	return out


def pack(problems):
	"""Time-major packing for the device: rows of ``round_up(npix, 4)`` floats; returns ``P``, ``fit``, offsets, npix, ncad."""
	npix = np.array([p.P.shape[1] for p in problems], dtype='int32')
	ncad = np.array([p.P.shape[0] for p in problems], dtype='int32')
	if np.any(npix < 1) or np.any(npix > MAX_PIXELS):
		raise ValueError(f"every Halo problem needs 1 .. {MAX_PIXELS} pixels")
	pitch = (npix.astype('int64') + 3) // 4 * 4
	sizes = pitch * ncad
	offset = np.zeros(len(problems), dtype='int64')
	offset[1:] = np.cumsum(sizes)[:-1]
	P = np.zeros(max(int(sizes.sum()), 4), dtype='float32')
	for i, p in enumerate(problems):
		P[offset[i]:offset[i] + sizes[i]].reshape(ncad[i], pitch[i])[:, :npix[i]] = p.P
	fit = np.concatenate([np.asarray(p.fit, dtype='uint8') for p in problems]) if problems else np.zeros(0, 'uint8')
	return P, (fit if len(fit) else np.zeros(1, 'uint8')), offset, npix, ncad


def _as_problems(problems):
	return [p if isinstance(p, Problem) else Problem(None, None, np.asarray(p[0], dtype='float32'), np.asarray(p[1], dtype=bool))
		for p in problems]


def _host_ptr(a):
	return a.ctypes.data_as(ctypes.c_void_p)


def tvmin(ctx, problems, maxiter=SETTINGS['maxiter'], history=HISTORY, ftol=FTOL, gtol=GTOL):
	"""
	The TV-min weights of a batch of problems on the device (``tp_halo_tvmin``).  ``problems``: a list of :class:`Problem` or of
	``(P, fit)`` (P float32 ``(ncad, npix)`` with finite values, fit bool ``(ncad,)``).  Returns a dict: ``w`` (list of float64
	weight vectors), ``l`` (list of float64 light curves over all cadences of each problem), ``f``, ``iterations``, ``status``.
	"""
	probs = _as_problems(problems)
	n = len(probs)
	if n == 0:
		return {'w': [], 'l': [], 'f': np.zeros(0), 'iterations': np.zeros(0, 'int32'), 'status': np.zeros(0, 'int32')}
	P, fit, offset, npix, ncad = pack(probs)
	dP, dfit = ctx.array(P), ctx.array(fit)
	dw = ctx.empty((int(npix.sum()),), 'float64')
	dl = ctx.empty((max(int(ncad.sum()), 1),), 'float64')
	df = ctx.empty((n,), 'float64')
	dit = ctx.empty((n,), 'int32')
	dst = ctx.empty((n,), 'int32')
	ctx._check(ctx.lib.tp_halo_tvmin(ctx.handle, n, _host_ptr(offset), _host_ptr(npix), _host_ptr(ncad), dP.ptr, dfit.ptr, int(maxiter),
		int(history), float(ftol), float(gtol), dw.ptr, dl.ptr, df.ptr, dit.ptr, dst.ptr))
	w, lc = dw.to_host(), dl.to_host()
	wo = np.concatenate([[0], np.cumsum(npix)])
	co = np.concatenate([[0], np.cumsum(ncad)])
	out = {'w': [w[wo[i]:wo[i+1]] for i in range(n)], 'l': [lc[co[i]:co[i+1]] for i in range(n)], 'f': df.to_host(),
		'iterations': dit.to_host(), 'status': dst.to_host()}
	for a in (dP, dfit, dw, dl, df, dit, dst):
		a.free()
	return out


def objective(ctx, problems, thetas):
	"""``f`` (float64 per problem) and the gradient with respect to ``theta`` (list) at ``thetas`` (``tp_halo_objective``)."""
	probs = _as_problems(problems)
	n = len(probs)
	P, fit, offset, npix, ncad = pack(probs)
	theta = np.concatenate([np.asarray(t, dtype='float64') for t in thetas])
	if len(theta) != int(npix.sum()):
		raise ValueError("one theta of npix values per problem expected")
	dP, dfit, dth = ctx.array(P), ctx.array(fit), ctx.array(theta)
	df = ctx.empty((n,), 'float64')
	dg = ctx.empty((len(theta),), 'float64')
	ctx._check(ctx.lib.tp_halo_objective(ctx.handle, n, _host_ptr(offset), _host_ptr(npix), _host_ptr(ncad), dP.ptr, dfit.ptr, dth.ptr,
		df.ptr, dg.ptr))
	g = dg.to_host()
	wo = np.concatenate([[0], np.cumsum(npix)])
	f = df.to_host()
	for a in (dP, dfit, dth, df, dg):
		a.free()
	return f, [g[wo[i]:wo[i+1]] for i in range(n)]


def weightmap(shape, pix, w, median):
	"""``w / median(l)`` in the stamp, zero elsewhere: ``sum(wm * image) = corr_flux`` at every cadence of the segment."""
	wm = np.zeros(int(np.prod(shape)))
	wm[pix] = w / median
	return wm.reshape(shape)


def flux_err(weightmaps, seg, images_err, normfactor):
	"""halo_photometry.py:210-219: ``|normfactor| sqrt(nansum(wm_k^2 err_k^2))`` with the weight map of the cadence's segment."""
	T = images_err.shape[2]
	out = np.zeros(T)
	for k in range(T):
		if seg[k] < 0:
			continue
		out[k] = np.abs(normfactor) * np.sqrt(np.nansum(weightmaps[seg[k]]**2 * images_err[:, :, k].astype('float64')**2))
	return out


def photometry(ctx, images, images_err, quality, time, timecorr, cadenceno, mask, sector, normfactor, maxiter=SETTINGS['maxiter']):
	"""
	The extraction of :176-219 for one target: the problems of its segments, their weights on the device, the normalised light
	curve and the weight maps.  Returns a dict: ``corr_flux`` (NaN where a cadence has no value), ``flux``, ``flux_err``,
	``weightmap`` dict (``weightmap``, ``initial_cadence``, ``final_cadence``, ``sat_pixels`` lists, one entry per segment),
	``w`` / ``status`` / ``iterations`` / ``f`` per segment, ``split_times``, ``segments``.
	"""
	splits = split_times(sector, time, timecorr)
	seg = segments(time, splits)
	probs = build_problems(images, quality, mask, seg)
	if not probs or any(p.P.shape[1] == 0 for p in probs):
		raise ValueError("Halo photometry: no usable pixels in the pixel mask")
	res = tvmin(ctx, probs, maxiter=maxiter)
	T = images.shape[2]
	corr = np.full(T, np.nan)
	wms, first, last = [], [], []
	cadenceno = np.asarray(cadenceno)
	for k, p in enumerate(probs):
		fitted = res['l'][k][np.asarray(p.fit, dtype=bool)]
		med = np.median(fitted) if len(fitted) else np.nan
		if res['status'][k] != DEGENERATE:
			corr[p.cad] = res['l'][k] / med
		wms.append(weightmap(images.shape[:2], p.pix, res['w'][k], med))
		cads = cadenceno[seg == k]
		first.append(int(cads.min()) if len(cads) else 0)
		last.append(int(cads.max()) if len(cads) else 0)
	return {'corr_flux': corr, 'flux': corr * normfactor, 'flux_err': flux_err(wms, seg, np.asarray(images_err), normfactor),
		'weightmap': {'weightmap': wms, 'initial_cadence': first, 'final_cadence': last, 'sat_pixels': [0] * len(probs)},
		'w': res['w'], 'status': res['status'], 'iterations': res['iterations'], 'f': res['f'], 'split_times': splits, 'segments': seg}
