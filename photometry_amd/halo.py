# -*- coding: utf-8 -*-
"""
Halo photometry (photometry/halo/halo_photometry.py:86-265) on the device: the host layer.

Upstream the pixel weights come from the third-party ``halophot`` (``do_lc``, :179-196), which this engine does not have.  The
method implemented here is the published TV-min method (Pope et al. 2016, 2019) with the reference's settings, defined in
DESIGN.md ("Halo") and restated on the CPU in ``tests/halo_common.py``: non-negative pixel weights that sum to one
(``w = softmax(theta)``) chosen so that the total variation of the normalised light curve is minimal, by L-BFGS from uniform
weights.  Because the digits cannot be halophot's, the plugin is opt-in: ``[halo] enabled = true`` in the settings.

This module holds the host part of :99-173 (stamp size, pixel mask, split times, segments, the packing of the problems), the
batched optimiser entry :func:`tvmin` (``tp_halo_tvmin``, csrc/halo.hip), :func:`objective` (``tp_halo_objective``),
:func:`photometry`, the whole light-curve extraction of one target that ``plugins.HaloPhotometry`` calls, and
:func:`photometry_frames`, the same for a batch of targets of a CCD region whose frames are resident on the device: the problems
are built there from the stack (``tp_halo_select_stack``, ``tp_halo_gather_stack``), one ``tp_halo_tvmin`` call serves the batch and
the outputs are formed there too (``tp_halo_outputs_stack``) -- no pixel value passes through the host.  :func:`photometry_cubes` is
the same for a group of target pixel files whose time-fastest cubes are on the device, every target with its own time axis, flags and
segments (``tp_halo_select_cubes``, ``tp_halo_gather_cubes``, ``tp_halo_outputs_cubes``; csrc/halo_cubes.hip).
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


# -- the batched path: problems built on the device from a region's frame stack ---------------------------------------------------
def frames_stamps(limits, targets):
	"""The Halo stamp of every target as the plugin forms it (:99-102): a fresh default stamp, then ``resize_stamp(width=22,
	height=22)``, clipped to ``limits``.  Returns int64 ``(n, 4)`` and a bool vector, False where no stamp is left."""
	from . import stamps as st
	n = len(targets['starid'])
	out, valid = np.full((n, 4), -1, dtype='int64'), np.zeros(n, dtype=bool)
	for i in range(n):
		row, col = float(targets['row'][i]), float(targets['column'][i])
		try:
			first = st.default_stamp(row, col, float(targets['tmag'][i]), limits)
			out[i] = st.moved(first, limits, row, col, width=DIST_MAX + 2, height=DIST_MAX + 2)
			valid[i] = out[i, 1] > out[i, 0] and out[i, 3] > out[i, 2]
		except ValueError:
			pass
	return out, valid


def frames_pixel_masks(ctx, stack, stamps, rows, columns, quality):
	"""The pixel masks (:118-120) of a group of equally sized stamps: ``aperture & 1`` is the finite part of the region's sum image
	cropped to the stamp (``BasePhotometry.aperture``, FFI branch).  bool ``(n, H, W)``."""
	from . import engine
	stamps = np.asarray(stamps, dtype='int64')
	H, W = int(stamps[0, 1] - stamps[0, 0]), int(stamps[0, 3] - stamps[0, 2])
	d_st = ctx.array(stamps.astype('int32'))
	crop = engine.crop_sumimage(ctx, stack.sumimage_for(quality), d_st, H, W, stack.row0, stack.col0)
	finite = np.isfinite(crop.to_host()).reshape(len(stamps), H, W)
	crop.free()
	d_st.free()
	out = np.zeros((len(stamps), H, W), dtype=bool)
	for i, st in enumerate(stamps):
		cols, rws = np.meshgrid(np.arange(st[2] + 1, st[3] + 1, 1, dtype='int32'), np.arange(st[0] + 1, st[1] + 1, 1, dtype='int32'))
		out[i] = pixel_mask(finite[i], cols, rws, rows[i], columns[i])
	return out


class FramesProblems(object):
	"""
	The problems of a group of equally sized stamps, selected on the device (``tp_halo_select_stack``): problem ``q = target * n_seg
	+ segment``; ``npix`` / ``ncad`` on the host, the lists ``pix`` / ``cad`` / ``fit`` / ``cadpos`` on the device.  :meth:`gather`
	packs the problems of the usable targets (every segment with 1 .. 4096 pixels) for ``tp_halo_tvmin``.
	"""
	def __init__(self, ctx, stack, stamps, masks, seg, quality, minflux=SETTINGS['minflux'], bitmask=None):
		from .engine import TESS_DEFAULT_BITMASK
		self.ctx, self.stack = ctx, stack
		self.stamps = np.ascontiguousarray(stamps, dtype='int32').reshape(-1, 4)
		self.n = len(self.stamps)
		self.H, self.W = int(self.stamps[0, 1] - self.stamps[0, 0]), int(self.stamps[0, 3] - self.stamps[0, 2])
		self.T = stack.n_cad
		self.seg = np.ascontiguousarray(seg, dtype='int32')
		self.n_seg = int(self.seg.max()) + 1 if len(self.seg) and self.seg.max() >= 0 else 0
		if self.n_seg < 1:
			raise ValueError("Halo photometry: no cadence with a finite time")
		quality = np.ascontiguousarray(quality, dtype='int32')
		if len(self.seg) != self.T or len(quality) != self.T:
			raise ValueError('segments and quality must have one entry per frame of the stack')
		n_prob, HW = self.n * self.n_seg, self.H * self.W
		self.n_prob = n_prob
		d_mask = ctx.array(np.ascontiguousarray(masks, dtype='uint8').reshape(self.n, HW))
		self.pix = ctx.empty((n_prob, HW), 'int32')
		self.cad = ctx.empty((n_prob, self.T), 'int32')
		self.fit = ctx.empty((n_prob, self.T), 'uint8')
		self.cadpos = ctx.empty((self.n, self.T), 'int32')
		counts = ctx.empty((2, n_prob), 'int32')
		ctx._check(ctx.lib.tp_halo_select_stack(ctx.handle, stack.dev['images'].ptr, *self._geometry(), d_mask.ptr, self.n_seg, _host_ptr(self.seg),
			_host_ptr(quality), int(TESS_DEFAULT_BITMASK if bitmask is None else bitmask), float(minflux), self.pix.ptr, self.cad.ptr, self.fit.ptr,
			self.cadpos.ptr, counts.ptr, counts.ptr + 4 * n_prob))
		c = counts.to_host()
		self.npix, self.ncad = c[0].reshape(self.n, self.n_seg), c[1].reshape(self.n, self.n_seg)
		counts.free()
		d_mask.free()
		self.usable = np.all((self.npix >= 1) & (self.npix <= MAX_PIXELS), axis=1)
		self.P = self.fitc = None

	def _geometry(self):
		s = self.stack
		return (s.n_cad, s.n_rows, s.n_cols, s.row0, s.col0, self.n, _host_ptr(self.stamps), self.H, self.W)

	def gather(self):
		"""``P`` and the fit bytes of the usable targets' problems on the device, laid out as :func:`pack` does."""
		ctx = self.ctx
		self.index = np.ascontiguousarray(np.flatnonzero(np.repeat(self.usable, self.n_seg)), dtype='int32')
		self.run_npix = np.ascontiguousarray(self.npix.ravel()[self.index], dtype='int32')
		self.run_ncad = np.ascontiguousarray(self.ncad.ravel()[self.index], dtype='int32')
		pitch = (self.run_npix.astype('int64') + 3) // 4 * 4
		sizes = pitch * self.run_ncad
		self.offset = np.zeros(len(self.index), dtype='int64')
		self.offset[1:] = np.cumsum(sizes)[:-1]
		self.P = ctx.empty((max(int(sizes.sum()), 4),), 'float32')
		self.fitc = ctx.empty((max(int(self.run_ncad.sum()), 1),), 'uint8')
		ctx._check(ctx.lib.tp_halo_gather_stack(ctx.handle, self.stack.dev['images'].ptr, *self._geometry(), self.n_seg, self.pix.ptr, self.cad.ptr,
			self.fit.ptr, len(self.index), _host_ptr(self.index), _host_ptr(self.offset), _host_ptr(self.run_npix), _host_ptr(self.run_ncad),
			self.P.ptr, self.fitc.ptr))
		return self

	def to_host(self):
		"""The problems as the restatement lists them (for the tests): per problem ``pix``, ``cad``, ``fit`` and, after
		:meth:`gather`, the padded block of ``P`` (``None`` for the problems of an unusable target)."""
		pix, cad, fit = self.pix.to_host(), self.cad.to_host(), self.fit.to_host()
		P = None if self.P is None else self.P.to_host()
		run = {int(q): r for r, q in enumerate(self.index)} if P is not None else {}
		out = []
		for q in range(self.n_prob):
			npix, ncad = int(self.npix.ravel()[q]), int(self.ncad.ravel()[q])
			block = None
			if q in run:
				r = run[q]
				pitch = (npix + 3) // 4 * 4
				block = P[self.offset[r]:self.offset[r] + pitch * ncad].reshape(ncad, pitch)
			out.append({'pix': pix[q, :npix], 'cad': cad[q, :ncad], 'fit': fit[q, :ncad].astype(bool), 'P': block})
		return out

	def free(self):
		for a in (self.pix, self.cad, self.fit, self.cadpos, self.P, self.fitc):
			if a is not None:
				a.free()


def _frames_chunk(ctx, stack, stamps, masks, seg, quality, normfactor, maxiter, out, idx):
	"""select -> counts -> gather -> ONE tp_halo_tvmin -> outputs -> download for the targets ``idx`` (one stamp size)."""
	from .device import device_view
	fp = FramesProblems(ctx, stack, stamps, masks, seg, quality)
	n, n_seg, T, HW = fp.n, fp.n_seg, fp.T, fp.H * fp.W
	fp.gather()
	n_run = len(fp.index)
	n_w, n_c = int(fp.run_npix.sum()), int(fp.run_ncad.sum())
	# one block of float64 for everything that goes back: w, f, median, corr_flux, flux, flux_err, the weight maps
	sizes = (n_w, n_run, fp.n_prob, n * T, n * T, n * T, fp.n_prob * HW)
	starts = np.concatenate([[0], np.cumsum(sizes)])
	block = ctx.empty((max(int(starts[-1]), 1),), 'float64')
	d_w, d_f, d_med, d_corr, d_flux, d_err, d_wm = (device_view(ctx, block.ptr + 8 * int(a), (max(int(m), 1),), 'float64', base=block)
		for a, m in zip(starts[:-1], sizes))
	d_l = ctx.empty((max(n_c, 1),), 'float64')
	d_is = ctx.empty((2, max(n_run, 1)), 'int32')
	if n_run:
		ctx._check(ctx.lib.tp_halo_tvmin(ctx.handle, n_run, _host_ptr(fp.offset), _host_ptr(fp.run_npix), _host_ptr(fp.run_ncad), fp.P.ptr, fp.fitc.ptr,
			int(maxiter), int(HISTORY), float(FTOL), float(GTOL), d_w.ptr, d_l.ptr, d_f.ptr, d_is.ptr, d_is.ptr + 4 * n_run))
	nf = np.ascontiguousarray(normfactor, dtype='float64')
	ctx._check(ctx.lib.tp_halo_outputs_stack(ctx.handle, stack.dev['images_err'].ptr, *fp._geometry(), n_seg, _host_ptr(fp.seg), fp.pix.ptr,
		fp.cadpos.ptr, n_run, _host_ptr(fp.index), _host_ptr(fp.run_npix), _host_ptr(fp.run_ncad), fp.fitc.ptr, d_w.ptr, d_l.ptr,
		d_is.ptr + 4 * n_run, _host_ptr(nf), d_med.ptr, d_corr.ptr, d_flux.ptr, d_err.ptr, d_wm.ptr))
	host, ints = block.to_host(), d_is.to_host()
	w, f, med, corr, flux, err, wm = (host[int(a):int(a) + int(m)] for a, m in zip(starts[:-1], sizes))
	out['corr_flux'][idx], out['flux'][idx], out['flux_err'][idx] = corr.reshape(n, T), flux.reshape(n, T), err.reshape(n, T)
	wm = wm.reshape(n, n_seg, fp.H, fp.W)
	wo = np.concatenate([[0], np.cumsum(fp.run_npix)])
	r = 0
	for j, i in enumerate(idx):
		out['npix'][i], out['ncad'][i] = fp.npix[j], fp.ncad[j]
		out['usable'][i] = fp.usable[j]
		if not fp.usable[j]:
			continue
		out['weightmap'][i] = [np.array(wm[j, k]) for k in range(n_seg)]
		out['w'][i] = [np.array(w[wo[r + k]:wo[r + k + 1]]) for k in range(n_seg)]
		out['f'][i], out['iterations'][i], out['status'][i] = f[r:r + n_seg], ints[0, r:r + n_seg], ints[1, r:r + n_seg]
		r += n_seg
	for a in (block, d_l, d_is):
		a.free()
	fp.free()


def photometry_frames(ctx, stack, targets, time, quality, sector=None, timecorr=None, cadenceno=None, maxiter=SETTINGS['maxiter'],
	budget_bytes=None):
	"""
	:func:`photometry` for every target of a CCD region held in a ``pipeline.FrameStack``, without a host copy of any pixel: per
	target the Halo stamp and pixel mask as the plugin forms them, the split times and segments once per batch (``sector=None``:
	the gap rule; ``timecorr=None``: zeros; ``cadenceno=None``: ``arange(T)``), then per stamp size select -> counts -> gather ->
	one ``tp_halo_tvmin`` -> outputs -> one download.  A batch whose ``P`` could exceed ``budget_bytes`` (default: a quarter of the
	device's memory) runs in chunks of targets; every target's result is independent of the chunking, to the bit.

	Returns a dict of columns: ``stamp`` int64 ``(n, 4)``, ``valid`` (a stamp exists), ``usable`` (every segment has 1 .. 4096
	pixels), ``pixel_mask`` (list of bool images), ``corr_flux`` / ``flux`` / ``flux_err`` float64 ``(n, T)``, ``weightmap`` and ``w``
	(lists per target of one entry per segment), ``f`` / ``iterations`` / ``status`` / ``npix`` / ``ncad`` ``(n, n_seg)``,
	``initial_cadence`` / ``final_cadence`` (per segment), ``split_times``, ``segments``.
	"""
	from .plugins import mag2flux
	n, T = len(targets['starid']), stack.n_cad
	time = np.asarray(time, dtype='float64')
	timecorr = np.zeros(T) if timecorr is None else np.asarray(timecorr, dtype='float64')
	cadenceno = np.arange(T) if cadenceno is None else np.asarray(cadenceno)
	splits = split_times(-1 if sector is None else sector, time, timecorr)
	seg = segments(time, splits)
	n_seg = int(seg.max()) + 1 if len(seg) and seg.max() >= 0 else 0
	stamps, valid = frames_stamps(stack.limits, targets)
	rows, cols = np.asarray(targets['row'], dtype='float64'), np.asarray(targets['column'], dtype='float64')
	out = {'stamp': stamps, 'valid': valid, 'usable': np.zeros(n, dtype=bool), 'pixel_mask': [None] * n, 'weightmap': [None] * n, 'w': [None] * n,
		'corr_flux': np.full((n, T), np.nan), 'flux': np.full((n, T), np.nan), 'flux_err': np.zeros((n, T)),
		'f': np.full((n, n_seg), np.nan), 'iterations': np.zeros((n, n_seg), dtype='int32'), 'status': np.zeros((n, n_seg), dtype='int32'),
		'npix': np.zeros((n, n_seg), dtype='int32'), 'ncad': np.zeros((n, n_seg), dtype='int32'), 'split_times': splits, 'segments': seg,
		# (a segment may hold no cadence -- three split times and a gap in the frames: 0 then, as halo.photometry writes it)
		'initial_cadence': [int(cadenceno[seg == k].min()) if np.any(seg == k) else 0 for k in range(n_seg)],
		'final_cadence': [int(cadenceno[seg == k].max()) if np.any(seg == k) else 0 for k in range(n_seg)]}
	if n_seg == 0:
		return out
	# (one scalar call per target, as the plugin makes it: the array form of the power function may round differently)
	normfactor = np.array([mag2flux(t) for t in np.asarray(targets['tmag'], dtype='float64')], dtype='float64')
	if budget_bytes is None:
		budget_bytes = ctx.info()['hbm_bytes'] / 4.0
	active = np.flatnonzero(valid)
	keys = (stamps[active, 1] - stamps[active, 0]) * 100000 + (stamps[active, 3] - stamps[active, 2])
	for key in np.unique(keys):
		idx = active[keys == key]
		HW = int(key // 100000) * int(key % 100000)
		masks = frames_pixel_masks(ctx, stack, stamps[idx], rows[idx], cols[idx], quality)
		# the most P a target can need: every cadence with a segment, every stamp pixel
		bound = 4.0 * ((HW + 3) // 4 * 4) * int(np.count_nonzero(seg >= 0))
		per = max(1, min(len(idx), int(budget_bytes // bound), 65535 // n_seg))
		for a in range(0, len(idx), per):
			sub = idx[a:a + per]
			for j, i in enumerate(sub):
				out['pixel_mask'][i] = masks[a + j]
			_frames_chunk(ctx, stack, stamps[sub], masks[a:a + per], seg, quality, normfactor[sub], maxiter, out, sub)
	return out


# -- the batched path for target pixel files: problems built on the device from a group's time-fastest cubes ------------------------
def _cubes_chunk(ctx, images, images_err, a, b, chosen, masks, segs, quality, normfactor, maxiter, out, minflux=SETTINGS['minflux'], bitmask=None):
	"""select -> counts -> gather -> ONE tp_halo_tvmin -> outputs -> download for the slots ``chosen`` of a group's cubes.  The call
	covers the slots ``[a, b)``; a slot in between that was not chosen travels as one problem without mask pixel or cadence."""
	from .device import device_view
	from .engine import TESS_DEFAULT_BITMASK
	m, T, H, W = b - a, images.n_cad, images.height, images.width
	HW = H * W
	seg = np.full((m, T), -1, dtype='int32')
	mask = np.zeros((m, HW), dtype='uint8')
	qual = np.zeros((m, T), dtype='int32')
	n_seg = np.ones(m, dtype='int32')
	for i in chosen:
		k = int(segs[i].max()) + 1 if len(segs[i]) and segs[i].max() >= 0 else 0
		if k < 1:
			continue                                                       # no cadence with a finite time: no problem, not usable
		seg[i - a], qual[i - a], n_seg[i - a] = segs[i], quality[i], k
		mask[i - a] = np.asarray(masks[i], dtype='uint8').ravel()
	prob_off = np.concatenate([[0], np.cumsum(n_seg)]).astype('int32')
	n_prob = int(prob_off[-1])
	cube, cube_err = images.slice0(a, m), images_err.slice0(a, m)
	geometry = (m, H, W, T, cube.t_pitch)
	d_mask = ctx.array(mask)
	pix, cad, fit = ctx.empty((n_prob, HW), 'int32'), ctx.empty((n_prob, T), 'int32'), ctx.empty((n_prob, T), 'uint8')
	cadpos = ctx.empty((m, T), 'int32')
	counts = ctx.empty((2, n_prob), 'int32')
	ctx._check(ctx.lib.tp_halo_select_cubes(ctx.handle, cube.ptr, *geometry, d_mask.ptr, _host_ptr(prob_off), _host_ptr(seg), _host_ptr(qual),
		int(TESS_DEFAULT_BITMASK if bitmask is None else bitmask), float(minflux), pix.ptr, cad.ptr, fit.ptr, cadpos.ptr, counts.ptr, counts.ptr + 4 * n_prob))
	c = counts.to_host()
	npix, ncad = c[0], c[1]
	counts.free()
	d_mask.free()
	usable = np.zeros(m, dtype=bool)
	for i in chosen:
		q0, q1 = prob_off[i - a], prob_off[i - a + 1]
		usable[i - a] = bool(np.any(seg[i - a] >= 0)) and bool(np.all((npix[q0:q1] >= 1) & (npix[q0:q1] <= MAX_PIXELS)))
	index = np.ascontiguousarray(np.flatnonzero(np.repeat(usable, n_seg)), dtype='int32')
	run_npix, run_ncad = np.ascontiguousarray(npix[index], dtype='int32'), np.ascontiguousarray(ncad[index], dtype='int32')
	sizes = (run_npix.astype('int64') + 3) // 4 * 4 * run_ncad
	offset = np.zeros(len(index), dtype='int64')
	offset[1:] = np.cumsum(sizes)[:-1]
	n_run, n_w, n_c = len(index), int(run_npix.sum()), int(run_ncad.sum())
	P = ctx.empty((max(int(sizes.sum()), 4),), 'float32')
	fitc = ctx.empty((max(n_c, 1),), 'uint8')
	ctx._check(ctx.lib.tp_halo_gather_cubes(ctx.handle, cube.ptr, *geometry, _host_ptr(prob_off), pix.ptr, cad.ptr, fit.ptr, n_run, _host_ptr(index),
		_host_ptr(offset), _host_ptr(run_npix), _host_ptr(run_ncad), P.ptr, fitc.ptr))
	# one block of float64 for everything that goes back: w, f, median, corr_flux, flux, flux_err, the weight maps
	parts = (n_w, n_run, n_prob, m * T, m * T, m * T, n_prob * HW)
	starts = np.concatenate([[0], np.cumsum(parts)])
	block = ctx.empty((max(int(starts[-1]), 1),), 'float64')
	d_w, d_f, d_med, d_corr, d_flux, d_err, d_wm = (device_view(ctx, block.ptr + 8 * int(s), (max(int(k), 1),), 'float64', base=block)
		for s, k in zip(starts[:-1], parts))
	d_l = ctx.empty((max(n_c, 1),), 'float64')
	d_is = ctx.empty((2, max(n_run, 1)), 'int32')
	if n_run:
		ctx._check(ctx.lib.tp_halo_tvmin(ctx.handle, n_run, _host_ptr(offset), _host_ptr(run_npix), _host_ptr(run_ncad), P.ptr, fitc.ptr, int(maxiter),
			int(HISTORY), float(FTOL), float(GTOL), d_w.ptr, d_l.ptr, d_f.ptr, d_is.ptr, d_is.ptr + 4 * n_run))
	nf = np.ascontiguousarray(normfactor[a:b], dtype='float64')
	ctx._check(ctx.lib.tp_halo_outputs_cubes(ctx.handle, cube_err.ptr, *geometry, _host_ptr(prob_off), _host_ptr(seg), pix.ptr, cadpos.ptr, n_run,
		_host_ptr(index), _host_ptr(run_npix), _host_ptr(run_ncad), fitc.ptr, d_w.ptr, d_l.ptr, d_is.ptr + 4 * n_run, _host_ptr(nf), d_med.ptr, d_corr.ptr,
		d_flux.ptr, d_err.ptr, d_wm.ptr))
	host, ints = block.to_host(), d_is.to_host()
	w, f, med, corr, flux, err, wm = (host[int(s):int(s) + int(k)] for s, k in zip(starts[:-1], parts))
	corr, flux, err, wm = corr.reshape(m, T), flux.reshape(m, T), err.reshape(m, T), wm.reshape(n_prob, H, W)
	wo = np.concatenate([[0], np.cumsum(run_npix)])
	run_of = np.full(n_prob, -1, dtype='int64')
	run_of[index] = np.arange(n_run)
	for i in chosen:
		j = i - a
		q0, q1 = int(prob_off[j]), int(prob_off[j + 1])
		if not np.any(seg[j] >= 0):
			continue
		out['corr_flux'][i], out['flux'][i], out['flux_err'][i] = corr[j], flux[j], err[j]
		out['npix'][i], out['ncad'][i], out['usable'][i] = npix[q0:q1].copy(), ncad[q0:q1].copy(), usable[j]
		out['median'][i] = med[q0:q1].copy()
		if not usable[j]:
			continue
		r = int(run_of[q0])
		k = q1 - q0
		out['weightmap'][i] = [np.array(wm[q]) for q in range(q0, q1)]
		out['w'][i] = [np.array(w[wo[r + s]:wo[r + s + 1]]) for s in range(k)]
		out['f'][i], out['iterations'][i], out['status'][i] = f[r:r + k].copy(), ints[0, r:r + k].copy(), ints[1, r:r + k].copy()
	for arr in (block, d_l, d_is, P, fitc, pix, cad, fit, cadpos):
		arr.free()


def photometry_cubes(ctx, group_cubes, masks, time, timecorr, cadenceno, quality, sector, normfactor, maxiter=SETTINGS['maxiter'],
	budget_bytes=None, targets=None):
	"""
	:func:`photometry` for the targets of a group of target pixel files whose cubes are resident on the device (``tpf.TpfGroup.cubes``:
	``images`` and ``images_err``, :class:`~photometry_amd.device.DeviceCube` s of ``n`` targets with one stamp shape and one number of
	cadences ``T``), without a host copy of any pixel: the analogue of :func:`photometry_frames`.  ``masks``: bool ``(n, H, W)`` pixel
	masks; ``time`` / ``timecorr`` / ``cadenceno`` / ``quality``: ``(n, T)``, one row per target -- the files share a shape, not their
	time axes, flags or gaps, so the split times and segments are every target's own (:func:`split_times`, :func:`segments`) and a
	batch mixes targets with one, two or more segments; ``sector`` / ``normfactor``: ``(n,)``.  ``targets``: the slots to run (default:
	all).  Per chunk select -> counts -> gather -> one ``tp_halo_tvmin`` for every usable problem -> outputs -> one download
	(``tp_halo_select_cubes``, ``tp_halo_gather_cubes``, ``tp_halo_outputs_cubes``).  A batch whose ``P`` could exceed ``budget_bytes``
	(default: a quarter of the device's memory) runs in chunks of targets; a target's result is independent of the chunking, to the bit.

	Returns a dict of columns over the ``n`` slots (``None`` / NaN for a slot that was not run): ``usable`` (every segment has 1 .. 4096
	pixels), ``corr_flux`` / ``flux`` / ``flux_err`` float64 ``(n, T)``, and per target ``weightmap`` and ``w`` (one entry per segment),
	``f`` / ``iterations`` / ``status`` / ``npix`` / ``ncad`` / ``median`` (arrays over its segments; ``median``: numpy's median of the
	segment's light curve over its fitted cadences, NaN for a target that is not usable), ``messages`` (what :func:`split_times` logged
	at WARNING level for the target, as ``"LEVEL: message"``: the plugin keeps these in its details), ``initial_cadence`` / ``final_cadence``,
	``split_times``, ``segments``.
	"""
	images, images_err = group_cubes['images'], group_cubes['images_err']
	n, T, H, W = images.n_targets, images.n_cad, images.height, images.width
	if (images_err.n_targets, images_err.n_cad, images_err.height, images_err.width, images_err.t_pitch) != (n, T, H, W, images.t_pitch):
		raise ValueError("photometry_cubes: images and images_err must have one shape and pitch")
	if H * W > MAX_PIXELS:
		raise ValueError(f"every Halo problem needs 1 .. {MAX_PIXELS} pixels")
	time = np.asarray(time, dtype='float64').reshape(n, T)
	timecorr = np.asarray(timecorr, dtype='float64').reshape(n, T)
	cadenceno = np.asarray(cadenceno).reshape(n, T)
	quality = np.ascontiguousarray(quality, dtype='int32').reshape(n, T)
	masks = np.asarray(masks).reshape(n, H, W)
	sector = np.broadcast_to(np.asarray(sector), (n,))
	normfactor = np.ascontiguousarray(np.broadcast_to(np.asarray(normfactor, dtype='float64'), (n,)))
	chosen = np.arange(n) if targets is None else np.unique(np.asarray(targets, dtype='int64'))
	if len(chosen) and (chosen[0] < 0 or chosen[-1] >= n):
		raise IndexError("photometry_cubes: target outside the cubes")
	none = lambda: [None] * n
	out = {'usable': np.zeros(n, dtype=bool), 'corr_flux': np.full((n, T), np.nan), 'flux': np.full((n, T), np.nan), 'flux_err': np.zeros((n, T)),
		'weightmap': none(), 'w': none(), 'f': none(), 'iterations': none(), 'status': none(), 'npix': none(), 'ncad': none(), 'median': none(), 'messages': none(), 'split_times': none(),
		'segments': none(), 'initial_cadence': none(), 'final_cadence': none()}
	bound = {}
	from .plugins import _DetailLog
	for i in chosen:
		# (what split_times warns about goes into the target's messages, as the plugin's log handler keeps it)
		out['messages'][i] = []
		handler = _DetailLog(out['messages'][i])
		logger.addHandler(handler)
		try:
			splits = split_times(sector[i], time[i], timecorr[i])
		finally:
			logger.removeHandler(handler)
		seg = segments(time[i], splits)
		k = int(seg.max()) + 1 if len(seg) and seg.max() >= 0 else 0
		out['split_times'][i], out['segments'][i] = splits, seg
		# (a segment may hold no cadence: 0 then, as halo.photometry writes it)
		out['initial_cadence'][i] = [int(cadenceno[i][seg == s].min()) if np.any(seg == s) else 0 for s in range(k)]
		out['final_cadence'][i] = [int(cadenceno[i][seg == s].max()) if np.any(seg == s) else 0 for s in range(k)]
		out['npix'][i], out['ncad'][i], out['median'][i] = np.zeros(k, dtype='int32'), np.zeros(k, dtype='int32'), np.full(k, np.nan)
		out['f'][i], out['iterations'][i], out['status'][i] = np.full(k, np.nan), np.zeros(k, dtype='int32'), np.zeros(k, dtype='int32')
		if k > 64:
			raise ValueError("Halo photometry: more than 64 segments")
		# the most P the target can need (every cadence with a segment, every stamp pixel) and its problems
		bound[int(i)] = (4.0 * ((H * W + 3) // 4 * 4) * int(np.count_nonzero(seg >= 0)), max(k, 1))
	if budget_bytes is None:
		budget_bytes = ctx.info()['hbm_bytes'] / 4.0
	# chunks of chosen slots in rising order: P within the budget, at most 65535 problems with the slots in between
	a = 0
	while a < len(chosen):
		b, nbytes, probs = a, 0.0, 0
		while b < len(chosen):
			more = bound[int(chosen[b])]
			between = int(chosen[b] - chosen[b - 1] - 1) if b > a else 0
			if b > a and (nbytes + more[0] > budget_bytes or probs + between + more[1] > 65535):
				break
			nbytes, probs, b = nbytes + more[0], probs + between + more[1], b + 1
		sub = [int(i) for i in chosen[a:b]]
		_cubes_chunk(ctx, images, images_err, sub[0], sub[-1] + 1, sub, masks, out['segments'], quality, normfactor, maxiter, out)
		a = b
	return out
