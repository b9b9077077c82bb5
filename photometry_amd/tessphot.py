# -*- coding: utf-8 -*-
"""
``tessphot(method, **task)`` -- the entry point the schedulers call once per task (reference: photometry/tessphot.py:52-135;
call sites run_tessphot.py:153, run_tessphot_mpi.py:178) with the contract they rely on:

* ``method`` in ``{None, 'aperture', 'psf', 'linpsf', 'halo'}``, anything else -> ``ValueError("Invalid method: '...'")``;
* the return value is always an object with ``status``, ``method`` and ``_details`` -- also when the plugin could not even be
  constructed (then ``method == 'error'``, ``status == STATUS.ERROR``, the traceback in ``_details['errors']``);
* an exception anywhere in the plugin becomes ``STATUS.ERROR`` with the traceback appended to the details; ``KeyboardInterrupt`` /
  ``SystemExit`` become ``STATUS.ABORT``; a light curve is saved only for ``OK`` / ``WARNING``;
* ``method=None`` runs aperture photometry and then asks whether a bright target (``Tmag <= haloswitch.tmag_limit``, not a
  secondary TPF target) should have been done with Halo photometry instead: either the aperture run gave up on stamp resizes, or
  the final mask still carries more than ``haloswitch.flux_limit`` of the expected flux on the stamp edge.

``tessphot_batch`` / ``tessphot_frames`` are the throughput entries (not in the reference): a whole batch per device pass.
"""

import logging
import traceback
import numpy as np
from .status import STATUS
from .plugins import AperturePhotometry, PSFPhotometry, LinPSFPhotometry, HaloPhotometry, load_settings, mag2flux

#: method keyword -> plugin class (tessphot.py:122-127)
PLUGINS = {'aperture': AperturePhotometry, 'psf': PSFPhotometry, 'linpsf': LinPSFPhotometry, 'halo': HaloPhotometry}

#: the two ways the aperture plugin reports that it ran out of stamp (photometry.py:156, :168), as they appear in the details
_RESIZE_GAVE_UP = ('Too many stamp resizes.', 'Stamp resize hit limit. Haloswitch quick break.')


class FailedTask(object):
	"""Stands in for the photometry object when its constructor raised: what the scheduler can still store."""
	method = 'error'

	def __init__(self, tracebacks):
		self.status = STATUS.ERROR
		self._details = {'errors': list(tracebacks)} if tracebacks else {}


def run_plugin(plugin, *args, before_save=None, **kwargs):
	"""Construct ``plugin``, run its photometry inside its context manager, save on success; never raises (see module doc).
	``before_save(pho)``: called after the photometry and before the light curve is written (a last word on status and details,
	so that the file on disk and the returned object agree)."""
	logger = logging.getLogger(__name__)
	pho, lost = None, []
	try:
		pho = plugin(*args, **kwargs)
		with pho:
			pho.photometry()
			if before_save is not None:
				before_save(pho)
			if pho.status in (STATUS.OK, STATUS.WARNING):
				pho.save_lightcurve()
	except (KeyboardInterrupt, SystemExit): # pragma: no cover
		logger.info("Stopped by user or system")
		if pho is not None:
			pho._status = STATUS.ABORT
	except BaseException: # noqa: B902 -- the scheduler must get a result for every task
		logger.exception("Something happened")
		text = traceback.format_exc().strip()
		if pho is not None:
			pho._status = STATUS.ERROR
			pho.report_details(error=text)
		else:
			lost.append(text)
	return FailedTask(lost) if pho is None else pho


#: the two reasons of the switch (tessphot.py:94, :101), by the code :func:`halo_switch_codes` returns
_SWITCH_TEXT = {1: "Too many stamp resizes. Let us try Halo instead.", 2: "Target is still touching the edge. Let us try Halo instead."}


def halo_switch_codes(tmag, is_tpf, failed, is_error, gave_up, edge_flux, tmag_limit, flux_limit):
	"""
	The predicate of tessphot.py:81-102 on columns (arrays of one length): ``tmag``, ``is_tpf`` (a ``tpf:`` datasource), ``failed``
	(the task never produced a photometry object), ``is_error`` (status ERROR), ``gave_up`` (one of the two resize messages is among
	the details' errors), ``edge_flux`` (NaN: none).  Returns int8: 0 no switch, else a key of the reasons.  The one predicate of
	the per-target entry (:func:`halo_switch_reason`) and of the batched one (:func:`tessphot_frames`).
	"""
	# (the expected flux and the ratio one scalar at a time, in the operands' own types: the expressions of tessphot.py:98-99 as the
	# per-target entry has always evaluated them -- the array form of the power function may round differently)
	tmag, edge_flux = list(tmag), list(edge_flux)
	with np.errstate(invalid='ignore', divide='ignore'):
		edge = np.array([bool(e / mag2flux(t) > flux_limit) for e, t in zip(edge_flux, tmag)], dtype=bool)
		faint = np.array([bool(t > tmag_limit) for t in tmag], dtype=bool)
	bright = ~np.asarray(failed, dtype=bool) & ~faint & ~np.asarray(is_tpf, dtype=bool)
	resize = np.asarray(is_error, dtype=bool) & np.asarray(gave_up, dtype=bool)
	return np.where(bright & resize, 1, np.where(bright & edge, 2, 0)).astype('int8')


def halo_switch_reason(pho, settings=None):
	"""
	Why the aperture result ``pho`` of a bright target should be redone with Halo photometry, or ``None``
	(the predicate of tessphot.py:81-102, :func:`halo_switch_codes` on one record).
	"""
	if isinstance(pho, FailedTask):
		return None
	settings = load_settings() if settings is None else settings
	messages = pho._details.get('errors', [])
	edge_flux = pho._details.get('edge_flux')
	code = halo_switch_codes([pho.target['tmag']], [pho.datasource.startswith('tpf:')], [False], [pho.status == STATUS.ERROR],
		[any(m in messages for m in _RESIZE_GAVE_UP)], [float('nan') if edge_flux is None else edge_flux],
		settings.getfloat('haloswitch', 'tmag_limit'), settings.getfloat('haloswitch', 'flux_limit'))[0]
	return _SWITCH_TEXT.get(int(code))


def tessphot(method=None, *args, **kwargs):
	"""Run the photometry pipeline on a single star; see the module documentation for the contract."""
	logger = logging.getLogger(__name__)
	if method is not None:
		if method not in PLUGINS:
			raise ValueError(f"Invalid method: '{method:s}'")
		pho = run_plugin(PLUGINS[method], *args, **kwargs)
	else:
		halo_on = HaloPhotometry.is_available()

		def keep_aperture_result(p):
			# Halo photometry off (the default, see HaloPhotometry): the finished aperture result is kept, not thrown away for a
			# plugin that can only fail; a good light curve is downgraded to WARNING and the request recorded BEFORE the light
			# curve is written, so that the file and the returned status agree.
			why = halo_switch_reason(p)
			if why is not None and not halo_on:
				p.report_details(error='Halo switch requested (' + why + ') but Halo photometry is not available: aperture result kept')
				if p.status == STATUS.OK:
					p._status = STATUS.WARNING

		pho = run_plugin(AperturePhotometry, *args, before_save=keep_aperture_result, **kwargs)
		reason = halo_switch_reason(pho)
		if reason is not None:
			logger.warning(reason)
			edge_flux = pho._details.get('edge_flux')
			if halo_on:
				pho = run_plugin(HaloPhotometry, *args, **kwargs)
				if isinstance(pho, HaloPhotometry):
					# keep the diagnostics that led to the switch (tessphot.py:104-109)
					pho.report_details('Automatically switched to Halo photometry')
					pho._details['edge_flux'] = edge_flux
		if pho.status == STATUS.WARNING:
			logger.warning("Do something else?")
	logger.info("Done")
	return pho


class BatchResult(object):
	"""What the scheduler consumes per target (taskmanager.py:444-563): status, method, details (+ the light curve)."""
	def __init__(self, starid, status, method, details, lightcurve, mask):
		self.starid = starid
		self.status = status
		self.method = method
		self._details = details
		self.lightcurve = lightcurve
		self.final_phot_mask = mask
		#: the weight maps of a target done with Halo photometry (``halo.photometry``'s ``weightmap`` dict), else None
		self.halo_weightmap = None


def _diagnostics_into(details, d, status):
	"""Copy the device diagnostics into ``details`` the way ``BasePhotometry.photometry`` does (BasePhotometry.py:1343-1407);
	returns the status, turned into ERROR where the reference raises ``ValueError``."""
	problems = int(d['flags'])
	if problems & 3:
		details.setdefault('errors', []).append('ValueError: Final lightcurve fluxes are all NaNs' if problems & 1
			else 'ValueError: Final lightcurve errors are all NaNs')
		return STATUS.ERROR
	if problems & 4:
		details.setdefault('errors', []).append('ValueError: Invalid time-vector specified')
		return STATUS.ERROR
	for key in ('mean_flux', 'variance', 'rms_hour', 'ptp', 'variability', 'edge_flux'):
		details[key] = float(d[key])
	details['pos_centroid'] = np.array([d['pos_centroid_col'], d['pos_centroid_row']])
	if problems & 8:
		details.setdefault('errors', []).append('WARNING: Could not detrend lightcurve for variability calculation.')
	if problems & 16:
		# the device's hourly binning gave up (unsorted or extremely sparse time axis): rms_hour is NaN -- say so
		details.setdefault('errors', []).append('WARNING: rms_hour not computed: the time axis could not be binned on the device.')
	return status


class BatchResults(object):
	"""
	What :func:`tessphot_frames` returns: the results of a whole batch in columns (``status`` int32 with the reference's STATUS
	integers -- what ``todolist.status`` stores, taskmanager.py:538-541 --, ``starid``, ``stamp``, ``stamp_resizes`` and, through
	:meth:`column`, ``mask_size`` / ``contamination`` / the diagnostics), and the per-target objects a scheduler's ``save_result``
	takes only when asked for: ``results[i]`` (or iteration) builds the :class:`BatchResult` of target ``i``.
	For a target that was switched to Halo photometry ``status`` and ``stamp`` are the Halo run's; ``stamp_resizes`` and
	:meth:`column` keep reporting the aperture run that led to the switch (the Halo values are in ``results[i]`` and ``self.halo``).
	"""

	def __init__(self, frames_result, starid):
		self.frames = frames_result
		self.starid = np.asarray(starid, dtype='int64')
		fr = frames_result
		status = fr.status.copy()
		# BasePhotometry.photometry (BasePhotometry.py:1343-1407): the diagnostics' ValueErrors turn OK / WARNING into ERROR
		self._problems = np.zeros(len(fr), dtype='int64')
		sel = np.flatnonzero(fr.has_result & ((status == STATUS.OK.value) | (status == STATUS.WARNING.value)))
		if len(sel):
			self._problems[sel] = fr.column('flags', fill=0)[sel].astype('int64')
			status[sel[(self._problems[sel] & 7) != 0]] = STATUS.ERROR.value
		self.status = status
		#: targets redone with Halo photometry (:meth:`switch_to_halo`): target -> row of ``self.halo``
		self.halo, self.halo_rows, self._stamp = None, {}, None
		#: ``(N, T, 2)`` changes in column and row of every target's position (``lightcurve['pos_corr']``, BasePhotometry.py:473) when
		#: the entry was given movement kernels, else None
		self.pos_corr = None
		#: the stack and the ``targets`` dict the batch was run over (set by :func:`tessphot_frames`): what :meth:`save_lightcurves` reads
		#: the pixel flags, the sum image and ``tmag`` from.  The results keep the stack, and its HBM, alive.
		self.stack = self.targets = None
		#: path of every target's light-curve file once :meth:`save_lightcurves` has run (``None``: no file), else None
		self.filepaths = None
		self._filepath_rel = {}

	def __len__(self):
		return len(self.frames)

	def save_lightcurves(self, output_folder, info, time, quality, version, *, timecorr=None, cadenceno=None, targets=None, workers=None, compresslevel=9):
		"""
		Write ``tess…-tasoc_lc.fits.gz`` for every target whose final status is OK or WARNING (the rule of :func:`run_plugin`): the file
		``tessphot('aperture', ...)`` -- or, for a target switched to Halo photometry, ``tessphot(None, ...)`` -- writes for it, into
		``output_folder`` under the reference's name (:mod:`photometry_amd.lcfile`).  ``info``: a :class:`~photometry_amd.lcfile.FileInfo`;
		``time`` / ``quality`` / ``timecorr`` / ``cadenceno``: the shared vectors of the batch (``TIME``, ``PIXEL_QUALITY``, ``TIMECORR``,
		``CADENCENO``; rows without a finite time are dropped from every column); ``targets``: the batch's ``targets`` dict (default: the
		one the entry was called with), which may carry the catalogue columns ``ra_J2000, decl_J2000, pm_ra, pm_decl, teff``.
		``QUALITY`` comes from the stack's pixel flags over the final stamps of the whole batch in one launch (all zero for a stack
		without flags).  ``workers`` threads (default ``min(16, os.cpu_count())``, never more than 16) build and compress the files;
		``compresslevel`` is gzip's (9: what the per-target plugin writes with).  Returns the paths, ``None`` where no file was written
		(also ``self.filepaths``); ``results[i]._details['filepath_lightcurve']`` is set as the plugin sets it.
		"""
		from . import lcfile
		if self.stack is None:
			raise ValueError("these results do not know their frame stack: run the batch through tessphot_frames")
		return lcfile.save_lightcurves(self, self.stack, output_folder, info, time, quality, version, timecorr=timecorr, cadenceno=cadenceno,
			targets=self.targets if targets is None else targets, workers=workers, compresslevel=compresslevel)

	def edge_flux_column(self):
		"""``details['edge_flux']`` of every target as a column (NaN: none): the flux on the stuck edge of the haloswitch quick break,
		else the diagnostics' edge flux of a finished light curve -- what :meth:`__getitem__` puts into the details."""
		fr = self.frames
		out = np.full(len(fr), np.nan)
		for i, v in fr.edge_flux.items():
			out[i] = v
		sel = np.flatnonzero(fr.has_result & ((fr.status == STATUS.OK.value) | (fr.status == STATUS.WARNING.value)) & ((self._problems & 7) == 0))
		if len(sel):
			out[sel] = fr.column('edge_flux')[sel]
		return out

	def halo_switch(self, tmag, settings, datasource='ffi'):
		"""The targets the predicate of tessphot.py:81-102 sends to Halo photometry: indices and reason codes."""
		fr = self.frames
		gave_up = np.zeros(len(fr), dtype=bool)
		for i, messages in fr.errors.items():
			gave_up[i] = any(m in messages for m in _RESIZE_GAVE_UP)
		codes = halo_switch_codes(tmag, np.full(len(fr), datasource.startswith('tpf:')), np.zeros(len(fr), dtype=bool),
			self.status == STATUS.ERROR.value, gave_up, self.edge_flux_column(), settings.getfloat('haloswitch', 'tmag_limit'),
			settings.getfloat('haloswitch', 'flux_limit'))
		idx = np.flatnonzero(codes)
		return idx, codes[idx]

	def switch_to_halo(self, idx, halo_result):
		"""Targets ``idx`` are what ``halo_result`` (a ``pipeline.HaloFramesResult`` over exactly them) says: tessphot.py:95-109."""
		self._aperture_edge_flux = self.edge_flux_column()
		self.halo = halo_result
		self.halo_rows = {int(i): j for j, i in enumerate(idx)}
		status = np.array(halo_result.status, dtype='int32')
		# the diagnostics' ValueErrors turn OK into ERROR here too (as __init__ does for the aperture targets): the column and
		# results[i].status agree
		for j, d in enumerate(halo_result.diagnostics):
			if d is not None and status[j] in (STATUS.OK.value, STATUS.WARNING.value) and int(d['flags']) & 7:
				status[j] = STATUS.ERROR.value
		self.status[idx] = status
		self._stamp = np.array(self.frames.stamp, copy=True)
		self._stamp[idx] = halo_result.stamp

	def _halo_item(self, i):
		r = self.halo[self.halo_rows[i]]
		status = STATUS(r['status'])
		details = {'stamp': r['stamp']}
		errors = list(r['errors'])
		lc = mask = None
		if status == STATUS.OK:
			mask = r['pixel_mask']
			T = len(r['flux'])
			lc = {'flux': r['flux'], 'flux_err': r['flux_err'], 'flux_background': np.zeros(T), 'pos_centroid': r['pos_centroid']}
			if self.pos_corr is not None:
				lc['pos_corr'] = self.pos_corr[i]
			if r['skip_targets']:
				details['skip_targets'] = r['skip_targets']
			status = _diagnostics_into(details, r['diagnostics'], status)
			details['mask_size'] = int(mask.sum())
			errors += details.pop('errors', [])
		# the diagnostics that led to the switch are kept (tessphot.py:104-109)
		details['errors'] = errors + ['Automatically switched to Halo photometry']
		ef = self._aperture_edge_flux[i]
		details['edge_flux'] = None if np.isnan(ef) else float(ef)
		if i in self._filepath_rel:
			details['filepath_lightcurve'] = self._filepath_rel[i]
		out = BatchResult(int(self.starid[i]), status, 'halo', details, lc, mask)
		out.halo_weightmap = r['weightmap']
		return out

	def column(self, name):
		"""Per-target float64 column: ``mask_size``, ``contamination`` or one of ``engine.DIAGNOSTICS_COLUMNS``; NaN without a result."""
		return self.frames.column(name)

	@property
	def stamp(self):
		"""The final stamp of every target: the Halo stamp for a target that was switched to Halo photometry."""
		return self.frames.stamp if self._stamp is None else self._stamp

	@property
	def stamp_resizes(self):
		return self.frames.stamp_resizes

	def __getitem__(self, i):
		if self.halo_rows:
			i = int(i) + len(self) if int(i) < 0 else int(i)
			if i in self.halo_rows:
				return self._halo_item(i)
		r = self.frames[i]
		status = STATUS(r['status'])
		details = {'stamp': r.get('stamp'), 'stamp_resizes': r['stamp_resizes']}
		if r['errors']:
			details['errors'] = list(r['errors'])
		if 'edge_flux' in r:
			details['edge_flux'] = r['edge_flux']
		lc = mask = None
		if 'mask' in r:
			mask = r['mask']
			details['mask_size'] = int(mask.sum())
			if r['skip_targets']:
				details['skip_targets'] = r['skip_targets']
			if not np.isnan(r['contamination']):
				details['contamination'] = r['contamination']
			lc = {k: r[k] for k in ('flux', 'flux_err', 'flux_background', 'pos_centroid')}
			if self.pos_corr is not None:
				lc['pos_corr'] = self.pos_corr[int(i)]
			if status in (STATUS.OK, STATUS.WARNING):
				status = _diagnostics_into(details, r['diagnostics'], status)
		if self._filepath_rel:
			k = int(i) + len(self) if int(i) < 0 else int(i)
			if k in self._filepath_rel:
				details['filepath_lightcurve'] = self._filepath_rel[k]
		return BatchResult(int(self.starid[int(i)]), status, 'aperture', details, lc, mask)

	def __iter__(self):
		return (self[i] for i in range(len(self)))


def _halo_switch_frames(ctx, stack, results, targets, catalog, time, quality, settings, sector, timecorr, cadenceno):
	"""The method switch of ``tessphot(None, ...)`` (tessphot.py:76-109) for a finished aperture batch: with ``[halo] enabled`` the
	bright targets whose aperture run gave up or left flux on a stuck edge go through ``pipeline.halo_frames`` in one call."""
	from . import pipeline, halo
	settings = load_settings() if settings is None else settings
	if not halo.enabled(settings):
		return results
	logger = logging.getLogger(__name__)
	idx, codes = results.halo_switch(np.asarray(targets['tmag']), settings)
	if len(idx) == 0:
		return results
	for code in codes:
		logger.warning(_SWITCH_TEXT[int(code)])
	sub = {k: np.asarray(targets[k])[idx] for k in ('starid', 'tmag', 'row', 'column')}
	res = pipeline.halo_frames(ctx, stack, sub, catalog, time, quality, sector=sector, timecorr=timecorr, cadenceno=cadenceno, settings=settings)
	results.switch_to_halo(idx, res)
	return results


def _pos_corr(ctx, movement, targets, time, timecorr):
	"""``(N, T, 2)``: ``movement.jitter(time - timecorr, column, row)`` of every target (BasePhotometry.py:473), formed on the device."""
	t = np.asarray(time, dtype='float64')
	t = t if timecorr is None else t - np.asarray(timecorr, dtype='float64')
	if movement.ctx is None:
		movement.ctx = ctx
	return movement.jitter_many(t, targets['column'], targets['row']).to_host()


def _finish_batch(ctx, out, stack, targets, time, quality, timecorr, cadenceno, movement, output_folder, fileinfo, version):
	"""What both batched entries do with a batch after the method switch: ``pos_corr``, the stack and targets, the files when asked for."""
	if movement is not None:
		out.pos_corr = _pos_corr(ctx, movement, targets, time, timecorr)
	out.stack, out.targets = stack, targets
	if output_folder is not None:
		if fileinfo is None:
			raise ValueError("output_folder needs fileinfo (a photometry_amd.lcfile.FileInfo)")
		out.save_lightcurves(output_folder, fileinfo, time, quality, version, timecorr=timecorr, cadenceno=cadenceno)
	return out


def tessphot_frames(ctx, stack, targets, catalog, time, quality, settings=None, sector=None, timecorr=None, cadenceno=None, movement=None,
	output_folder=None, fileinfo=None, version=None):
	"""
	Aperture photometry of every target of a CCD region resident in HBM (:class:`photometry_amd.pipeline.FrameStack`), stamp
	resizes included: what ``tessphot('aperture', ...)`` returns per target, for the whole batch in a few device passes.
	With ``[halo] enabled = true`` in the settings it is ``tessphot(None, ...)``: the bright targets whose aperture run gave up on
	stamp resizes or left flux on a stuck edge (:func:`halo_switch_codes`) are redone with Halo photometry in one batched call
	(``pipeline.halo_frames``; ``sector`` / ``timecorr`` / ``cadenceno`` as there) and their results are the Halo ones
	(``method == 'halo'``, ``halo_weightmap``).
	``movement``: a :class:`~photometry_amd.motion.MovementKernel` with a loaded series: ``BatchResults.pos_corr`` and every light
	curve's ``'pos_corr'`` are then its jitter at the targets' positions at ``time - timecorr``, as the plugins write it.
	``output_folder`` with ``fileinfo`` (a :class:`~photometry_amd.lcfile.FileInfo`) and ``version``: the light-curve files of the batch
	are written as well (:meth:`BatchResults.save_lightcurves`), as ``run_plugin`` writes them per target.
	Returns a :class:`BatchResults`: columns for the whole batch, one :class:`BatchResult` per target on demand (``results[i]``).
	"""
	from . import pipeline
	res = pipeline.aperture_frames(ctx, stack, targets, catalog, time, quality, settings=settings)
	out = _halo_switch_frames(ctx, stack, BatchResults(res, targets['starid']), targets, catalog, time, quality, settings, sector, timecorr, cadenceno)
	return _finish_batch(ctx, out, stack, targets, time, quality, timecorr, cadenceno, movement, output_folder, fileinfo, version)


def tessphot_frames_pipelined(ctx, stack, batches, catalog, time, quality, settings=None, in_flight=4, sector=None, timecorr=None, cadenceno=None,
	movement=None, output_folder=None, fileinfo=None, version=None):
	"""
	:func:`tessphot_frames` over consecutive batches of targets of one CCD region -- what a run over a whole CCD does, a few
	thousand targets per call -- with ``in_flight`` batches on the device at a time (``pipeline.aperture_frames_pipelined``: the
	first round of a batch runs under the latency-bound resize rounds of the one before it).  ``batches``: an iterable of
	``targets`` dicts; yields one :class:`BatchResults` per batch, in order, equal to what a call of its own returns (the switch to
	Halo photometry included, applied to each batch before it is yielded; ``movement`` as there; with ``output_folder`` / ``fileinfo`` /
	``version`` the files of each batch are written as it is collected).
	"""
	from . import pipeline
	batches = list(batches) if not hasattr(batches, '__next__') else batches
	seen = []
	def feed():
		for t in batches:
			seen.append(t)
			yield t
	for k, res in enumerate(pipeline.aperture_frames_pipelined(ctx, stack, feed(), catalog, time, quality, settings=settings, in_flight=in_flight)):
		out = _halo_switch_frames(ctx, stack, BatchResults(res, seen[k]['starid']), seen[k], catalog, time, quality, settings, sector, timecorr, cadenceno)
		yield _finish_batch(ctx, out, stack, seen[k], time, quality, timecorr, cadenceno, movement, output_folder, fileinfo, version)


def tessphot_batch(ctx, scene, cubes='host'):
	"""
	Aperture photometry of a whole batch of FIXED-size stamp cubes in one pass over the device
	(``pipeline.run_aperture``); returns one :class:`BatchResult` per target, in order.
	``scene`` carries the arrays of ``photometry_amd.simulate.Scene`` (cubes, catalogue, positions).  A cube cannot grow:
	a mask that touches its edge is used as it is, like the reference does when ``resize_stamp`` returns False
	(BasePhotometry.py:605-612), and reported in ``details['edge']``; use :func:`tessphot_frames` when the frames the
	stamps were cut from are available, so that such targets get the reference's stamp-resize retries.
	"""
	from . import pipeline
	from .engine import DIAGNOSTICS_COLUMNS
	res = pipeline.run_aperture(ctx, scene, cubes=cubes)
	out = []
	for i in range(scene.n_targets):
		status = STATUS(int(res['status'][i]))
		flags = int(res['flags'][i])
		a, b = scene.cat_offsets[i], scene.cat_offsets[i+1]
		inm = res['cat_in_mask'][a:b].astype(bool)
		ids = scene.catalog['starid'][a:b][inm]
		details = {'stamp': tuple(int(v) for v in scene.stamps[i]), 'mask_size': int(res['mask'][i].sum())}
		skip = [int(s) for s in ids if s != scene.target_starid[i]]
		if skip:
			details['skip_targets'] = skip
		if not np.isnan(res['contamination'][i]):
			details['contamination'] = float(res['contamination'][i])
		if flags >> 8:
			details['errors'] = [f'ERROR: aperture mask creation failed (kind {flags >> 8})']
		if flags & 30:
			details['edge'] = flags & 30
			details.setdefault('errors', []).append('WARNING: Could not resize stamp any further.')  # photometry.py:141-144
		if status in (STATUS.OK, STATUS.WARNING):
			status = _diagnostics_into(details, dict(zip(DIAGNOSTICS_COLUMNS, res['diagnostics'][i])), status)
		lc = {k: res[k][i] for k in ('flux', 'flux_err', 'flux_background', 'pos_centroid')}
		out.append(BatchResult(int(scene.target_starid[i]), status, 'aperture', details, lc, res['mask'][i].astype(bool)))
	return out
