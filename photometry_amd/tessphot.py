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
``tessphot_tpfs`` is the one for target pixel files: ``tessphot('aperture', ..., datasource='tpf')`` for many files, one pass per group
of files that share stamp shape and number of cadences; with ``method=None`` or ``'halo'`` it is ``tessphot(None, ...)`` /
``tessphot('halo', ...)`` for them, the Halo problems built on the device from the group's cubes (``pipeline.halo_tpfs``), and with
``method='linpsf'`` ``tessphot('linpsf', ...)``, one fit per group on the cubes as they lie (``pipeline.linpsf_tpfs``).
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
		#: the header cards a method adds to its light-curve file where the batch knows them per target (LinPSF: ``PSF_FERR``, ``PSF_CONT``)
		self.additional_headers = {}


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
		self._halo_direct = False
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

	def save_lightcurves(self, output_folder, info, time, quality, version, *, timecorr=None, cadenceno=None, targets=None, workers=None, compresslevel=9, compress='zlib',
		table='host'):
		"""
		Write ``tess…-tasoc_lc.fits.gz`` for every target whose final status is OK or WARNING (the rule of :func:`run_plugin`): the file
		``tessphot('aperture', ...)`` -- or, for a target switched to Halo photometry, ``tessphot(None, ...)`` -- writes for it, into
		``output_folder`` under the reference's name (:mod:`photometry_amd.lcfile`).  ``info``: a :class:`~photometry_amd.lcfile.FileInfo`;
		``time`` / ``quality`` / ``timecorr`` / ``cadenceno``: the shared vectors of the batch (``TIME``, ``PIXEL_QUALITY``, ``TIMECORR``,
		``CADENCENO``; rows without a finite time are dropped from every column); ``targets``: the batch's ``targets`` dict (default: the
		one the entry was called with), which may carry the catalogue columns ``ra_J2000, decl_J2000, pm_ra, pm_decl, teff``.
		``QUALITY`` comes from the stack's pixel flags over the final stamps of the whole batch in one launch (all zero for a stack
		without flags).  ``workers`` threads (default ``min(16, os.cpu_count())``, never more than 16) build and compress the files;
		``compresslevel`` is gzip's (9: what the per-target plugin writes with).  ``compress='device'``: the workers build the bytes, the
		calling thread compresses them on the stack's device and the workers write the members (``lcfile.save_lightcurves``; the same
		content, other compressed bytes; ``compresslevel`` is ignored).  ``table='device'`` (with ``compress='device'`` only; anything else
		raises ``ValueError``): the ``LIGHTCURVE`` data units are written on the device with their DATASUMs straight into the encoder's input
		(``tp_lc_table_pack``) and the workers build headers and image HDUs only -- the same file bytes.  Returns the paths, ``None`` where no file was written
		(also ``self.filepaths``); ``results[i]._details['filepath_lightcurve']`` is set as the plugin sets it.
		"""
		from . import lcfile
		if self.stack is None:
			raise ValueError("these results do not know their frame stack: run the batch through tessphot_frames")
		return lcfile.save_lightcurves(self, self.stack, output_folder, info, time, quality, version, timecorr=timecorr, cadenceno=cadenceno,
			targets=self.targets if targets is None else targets, workers=workers, compresslevel=compresslevel, compress=compress, table=table)

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
		if self._halo_direct:
			# Halo photometry was asked for (``method='halo'``): nothing was switched, the details are the Halo run's alone
			if errors:
				details['errors'] = errors
		else:
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


def _finish_batch(ctx, out, stack, targets, time, quality, timecorr, cadenceno, movement, output_folder, fileinfo, version, compress='zlib', table='host'):
	"""What both batched entries do with a batch after the method switch: ``pos_corr``, the stack and targets, the files when asked for."""
	if movement is not None:
		out.pos_corr = _pos_corr(ctx, movement, targets, time, timecorr)
	out.stack, out.targets = stack, targets
	if output_folder is not None:
		if fileinfo is None:
			raise ValueError("output_folder needs fileinfo (a photometry_amd.lcfile.FileInfo)")
		out.save_lightcurves(output_folder, fileinfo, time, quality, version, timecorr=timecorr, cadenceno=cadenceno, compress=compress, table=table)
	return out


def tessphot_frames(ctx, stack, targets, catalog, time, quality, settings=None, sector=None, timecorr=None, cadenceno=None, movement=None,
	output_folder=None, fileinfo=None, version=None, compress='zlib', table='host'):
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
	are written as well (:meth:`BatchResults.save_lightcurves`), as ``run_plugin`` writes them per target; ``compress``: ``'zlib'`` or
	``'device'``, and ``table``: ``'host'`` or ``'device'``, as there.
	Returns a :class:`BatchResults`: columns for the whole batch, one :class:`BatchResult` per target on demand (``results[i]``).
	"""
	from . import pipeline, lcfile
	lcfile._check_table(table, compress)
	res = pipeline.aperture_frames(ctx, stack, targets, catalog, time, quality, settings=settings)
	out = _halo_switch_frames(ctx, stack, BatchResults(res, targets['starid']), targets, catalog, time, quality, settings, sector, timecorr, cadenceno)
	return _finish_batch(ctx, out, stack, targets, time, quality, timecorr, cadenceno, movement, output_folder, fileinfo, version, compress, table)


def tessphot_frames_pipelined(ctx, stack, batches, catalog, time, quality, settings=None, in_flight=4, sector=None, timecorr=None, cadenceno=None,
	movement=None, output_folder=None, fileinfo=None, version=None, compress='zlib', table='host'):
	"""
	:func:`tessphot_frames` over consecutive batches of targets of one CCD region -- what a run over a whole CCD does, a few
	thousand targets per call -- with ``in_flight`` batches on the device at a time (``pipeline.aperture_frames_pipelined``: the
	first round of a batch runs under the latency-bound resize rounds of the one before it).  ``batches``: an iterable of
	``targets`` dicts; yields one :class:`BatchResults` per batch, in order, equal to what a call of its own returns (the switch to
	Halo photometry included, applied to each batch before it is yielded; ``movement`` as there; with ``output_folder`` / ``fileinfo`` /
	``version`` the files of each batch are written as it is collected, ``compress`` and ``table`` as there).
	"""
	from . import pipeline, lcfile
	lcfile._check_table(table, compress)
	batches = list(batches) if not hasattr(batches, '__next__') else batches
	seen = []
	def feed():
		for t in batches:
			seen.append(t)
			yield t
	for k, res in enumerate(pipeline.aperture_frames_pipelined(ctx, stack, feed(), catalog, time, quality, settings=settings, in_flight=in_flight)):
		out = _halo_switch_frames(ctx, stack, BatchResults(res, seen[k]['starid']), seen[k], catalog, time, quality, settings, sector, timecorr, cadenceno)
		yield _finish_batch(ctx, out, stack, seen[k], time, quality, timecorr, cadenceno, movement, output_folder, fileinfo, version, compress, table)


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


#--------------------------------------------------------------------------------------------------
#: the share of the free device memory the three cubes of one chunk of :func:`tessphot_tpfs` may take, and the most files of a chunk
TPF_CHUNK_SHARE = 0.25
TPF_CHUNK_MAX = 4096


def tpf_chunk_files(shapes, free_bytes, share=TPF_CHUNK_SHARE, most=TPF_CHUNK_MAX):
	"""
	Files per chunk of :func:`tessphot_tpfs` from the header shapes ``(H, W, n_rows)``: as many of the largest file's three float32
	cubes (``H * W`` series of ``n_rows`` rounded up to 32 cadences) as fit ``share`` of ``free_bytes``; at least 1, at most ``most``
	and the number of files.
	"""
	per_file = max(3 * 4 * int(H) * int(W) * (-(-int(n_rows) // 32) * 32) for H, W, n_rows in shapes)
	return int(max(1, min(int(most), len(shapes), int(share * free_bytes) // per_file)))


class TpfBatchResults(BatchResults):
	"""
	What :func:`tessphot_tpfs` yields per chunk: :class:`BatchResults` over target pixel files.  ``starid``, ``status``, ``paths`` (the
	input files) and ``filepaths`` (the light-curve files, ``None`` where none was written or asked for) are in input order;
	``column(name)`` as there; ``results[i]`` is the :class:`BatchResult` the per-file call ``tessphot('aperture', starid,
	TpfStampSource(...), datasource='tpf')`` returns (with ``method=None`` / ``'halo'`` of the entry: what ``tessphot(None, ...)`` /
	``tessphot('halo', ...)`` returns; ``halo_rows``, ``halo`` and ``halo_requests`` say which targets were switched, to what, or would have
	been with Halo photometry on; with ``method='linpsf'``: what ``tessphot('linpsf', ...)`` returns, ``linpsf`` holds the groups'
	``pipeline.LinPSFTpfsResult`` s): its light curve carries ``time, timecorr, cadenceno, quality`` and ``pos_corr``
	(``POS_CORR1/2``) of the file besides the photometry.  ``stamp_resizes`` is 0 throughout (a ``tpf`` stamp is the whole file) and is
	kept in the details, as on :class:`BatchResults`; where the diagnostics raise upstream the details carry that error alone, as the
	plugin's do.  ``loaded``: the ``tpf.LoadedTPF`` of every file (its cubes are gone once the chunk has been yielded).
	"""

	def __init__(self, frames_result, starid, tmag, paths, loaded, apertures):
		super().__init__(frames_result, starid)
		#: ``tmag`` of every file's main target
		self.tmag = np.asarray(tmag, dtype='float64')
		self.paths = list(paths)
		self.loaded = list(loaded)
		self._apertures = apertures
		self.filepaths = [None] * len(self.paths)
		#: the context the chunk was computed on (set by :func:`tessphot_tpfs`): where ``compress='device'`` runs
		self.ctx = None
		#: ``method=None`` with Halo photometry off: target -> the recorded request (:meth:`keep_aperture_results`)
		self.halo_requests = {}
		#: ``method='linpsf'``: the :class:`~photometry_amd.pipeline.LinPSFTpfsResult` of every group, target -> (part, row), and the files
		#: whose main target is not in the catalogue -> the error (:meth:`set_linpsf`); None for the other methods
		self.linpsf = None
		self._linpsf_where, self._linpsf_lost = {}, {}

	def set_linpsf(self, parts, where, lost):
		"""The chunk was run with ``method='linpsf'``: ``parts`` are the ``pipeline.linpsf_tpfs`` results of its groups, target ``i`` is row
		``where[i][1]`` of ``parts[where[i][0]]``; the targets of ``lost`` never got a photometry object (``lost[i]``: why)."""
		self.linpsf = list(parts)
		self._linpsf_where = {int(i): (int(p), int(j)) for i, (p, j) in where.items()}
		self._linpsf_lost = {int(i): str(text) for i, text in lost.items()}
		self.status[:] = STATUS.ERROR.value
		for i, (p, j) in self._linpsf_where.items():
			self.status[i] = self.linpsf[p].status[j]

	def _linpsf_item(self, i):
		"""What ``tessphot('linpsf', starid, TpfStampSource(...), datasource='tpf')`` returns for file ``i``."""
		if not 0 <= i < len(self):
			raise IndexError(i)
		if i not in self._linpsf_where:
			return BatchResult(int(self.starid[i]), STATUS.ERROR, 'linpsf', {'errors': [self._linpsf_lost[i]]}, None, None)
		p, j = self._linpsf_where[i]
		r = self.linpsf[p][j]
		status = STATUS(r['status'])
		details = {'stamp': r['stamp']}
		lc = None
		if r['fitted']:
			# (the fit ran: the plugin's light curve holds what it gave whatever became of the status; pos_centroid stays as created)
			T = len(r['flux'])
			lc = {'flux': r['flux'], 'flux_err': r['flux_err'], 'flux_background': np.zeros(T), 'pos_centroid': np.zeros((T, 2))}
		d = r['diagnostics']
		if d is not None and status in (STATUS.OK, STATUS.WARNING):
			for key in ('mean_flux', 'variance', 'rms_hour', 'ptp', 'variability'):
				details[key] = float(d[key])
			details['pos_centroid'] = np.array([d['pos_centroid_col'], d['pos_centroid_row']])
		if r['errors']:
			details['errors'] = list(r['errors'])
		if i in self._filepath_rel:
			details['filepath_lightcurve'] = self._filepath_rel[i]
		out = BatchResult(int(self.starid[i]), status, 'linpsf', details, lc, None)
		out.additional_headers = r['headers']
		return out

	def keep_aperture_results(self, idx, codes):
		"""The targets ``idx`` should have gone to Halo photometry (reasons ``codes``) but it is off: the aperture results are kept, the
		request is recorded in their errors and OK becomes WARNING -- what ``tessphot(None, ...)`` does before it saves the light curve."""
		for i, code in zip(idx, codes):
			self.halo_requests[int(i)] = 'Halo switch requested (' + _SWITCH_TEXT[int(code)] + ') but Halo photometry is not available: aperture result kept'
			if self.status[i] == STATUS.OK.value:
				self.status[i] = STATUS.WARNING.value

	def save_lightcurves(self, output_folder, version, workers=None, compresslevel=9, compress='zlib', table='host'):
		"""Write the light-curve file of every OK / WARNING target as the per-file plugin call does (``lcfile.save_tpf_lightcurves``);
		``compress='device'`` compresses on the context of the batch, by the calling thread; ``table='device'`` (with it only) writes the
		``LIGHTCURVE`` data units on the device as well, one ``tp_lc_table_pack`` per set of files with one length and one list of kept rows."""
		from . import lcfile
		return lcfile.save_tpf_lightcurves(self, output_folder, version, workers=workers, compresslevel=compresslevel, compress=compress, ctx=self.ctx, table=table)

	def aperture_image(self, i):
		"""The APERTURE image of file ``i`` without SPOC's mask and centroid flags: ``BasePhotometry.aperture`` of a ``tpf`` run."""
		return self._apertures[int(i)]

	def sumimage(self, i):
		i = int(i) + len(self) if int(i) < 0 else int(i)
		return np.array(self.frames.groups[self.frames.group[i]]['sumimage'][self.frames.pos[i]])

	def __getitem__(self, i):
		i = int(i) + len(self) if int(i) < 0 else int(i)
		out = self._linpsf_item(i) if self.linpsf is not None else super().__getitem__(i)
		if i not in self.halo_rows and (self._problems[i] & 7) and 'errors' in out._details:
			out._details['errors'] = out._details['errors'][-1:]       # (the plugin raises: what it had logged is lost, BasePhotometry.py:1346-1349)
		if i in self.halo_requests:
			# Halo photometry off: the aperture result is kept and the request recorded, as tessphot(None, ...) does before it saves
			out._details.setdefault('errors', []).append(self.halo_requests[i])
			out.status = STATUS(int(self.status[i]))
		if out.lightcurve is not None:
			ld = self.loaded[i]
			lc = {'time': np.array(ld.time, dtype='float64'), 'timecorr': np.array(ld.timecorr, dtype='float64'), 'cadenceno': np.array(ld.cadenceno),
				'quality': np.array(ld.quality)}
			lc.update({k: out.lightcurve[k] for k in ('flux', 'flux_err', 'flux_background', 'pos_centroid')})
			lc['pos_corr'] = np.array(ld.pos_corr, dtype='float64')
			out.lightcurve = lc
		return out


def _one_attempt(flags):
	"""What ``AperturePhotometry.do_photometry`` makes of the device flags of an attempt whose stamp cannot grow (a ``tpf`` run:
	photometry.py:113-170, :243-257): ``(status, has_result, messages)`` in the words of the plugin's log."""
	from .plugins import _MASK_EXCEPTIONS
	from . import stamps
	flags = int(flags)
	kind = flags >> 8
	if kind in _MASK_EXCEPTIONS:                                         # uncaught upstream: the traceback is all that is left
		return STATUS.ERROR, False, ['RuntimeError: ' + _MASK_EXCEPTIONS[kind]]
	messages = []
	if flags & 32:
		messages.append('ERROR: No flux above threshold.')
	if flags & 1:
		messages.append('WARNING: No masks found. Using minimum aperture.' if flags & (32 | 64) else 'WARNING: No mask found for main target. Using minimum aperture.')
	if kind == 5:
		return STATUS.ERROR, False, messages + ['ERROR: Too many masks.']
	if stamps.edge_requests(flags):
		messages.append('WARNING: Could not resize stamp any further.')
	status = STATUS.OK
	if kind == 6:
		messages.append('ERROR: No targets in mask.')
		status = STATUS.ERROR
	return (STATUS.WARNING if flags & 1 else status), True, messages


def _linpsf_tpfs_chunk(ctx, fr, groups, by_slot, cats, pos, lost, starid, files, loaded, prf, flux_errors):
	"""``method='linpsf'`` for a loaded chunk: per group the sum images the light-curve files carry (``tp_sumimage`` on the group's cube with
	every file's own quality row: the plugin's ``sumimage`` property) and one ``pipeline.linpsf_tpfs`` over the files whose main target is
	in the catalogue.  No aperture mask is made and nothing of the K2P2 / extraction pass is run."""
	from . import pipeline, engine
	n = len(files)
	apertures = [None] * n
	parts, where = [], {}
	for g, grp in enumerate(groups):
		ids = by_slot[g]
		d_quality = ctx.array(np.ascontiguousarray(grp.quality, dtype='int32'))
		d_sum = engine.sumimage(ctx, grp.cubes['images'], d_quality)
		fr.groups.append({'sumimage': d_sum.to_host()})
		d_sum.free()
		d_quality.free()
		for s, i in enumerate(ids):
			fr.group[i], fr.pos[i] = g, s
			apertures[i] = grp.aperture[s]
		slots = [s for s, i in enumerate(ids) if i not in lost]
		if not slots:
			continue
		chosen = [ids[s] for s in slots]
		res = pipeline.linpsf_tpfs(ctx, grp, slots, [cats[i] for i in chosen], pos[chosen], np.asarray(starid, dtype='int64')[chosen], prf, flux_errors=flux_errors)
		for j, i in enumerate(chosen):
			where[i] = (len(parts), j)
		parts.append(res)
	out = TpfBatchResults(fr, starid, pos[:, 2], files, loaded, apertures)
	out.set_linpsf(parts, where, lost)
	return out


def _tpf_chunk(ctx, files, headers, starid, catalog, targets, verify, method='aperture', settings=None, prf=None, linpsf_errors=False):
	"""One chunk of :func:`tessphot_tpfs`: load, one device pass per ``(H, W, T)`` group, the method switch, the results in input order."""
	from . import tpf, pipeline
	n = len(files)
	groups, index = tpf.load_tpf_groups(ctx, files, verify=verify, headers=headers)
	try:
		loaded = [groups[g].loaded[s] for g, s in index]
		stamps_all = np.array([ld.max_stamp for ld in loaded], dtype='int64').reshape(n, 4)
		cat_px, tgt_px = tpf.project_for_files(ctx, loaded, catalog, targets)
		shared = None
		if cat_px is None:
			shared = {k: np.asarray(catalog[k]) for k in ('starid', 'tmag', 'row', 'column')}
			offs_all, cat_all = pipeline._catalogs_of_stamps(pipeline._CatalogIndex(shared), stamps_all)
			first = {}
			for k, sid in enumerate(shared['starid']):
				first.setdefault(int(sid), k)
		tstar = None if targets is None else np.asarray(targets['starid'])
		# per file: the stars of its stamp and its main target, as TpfStampSource and BasePhotometry.__init__ make them
		cats, pos, lost = [], np.zeros((n, 3)), {}
		for i, ld in enumerate(loaded):
			r0, _, c0, _ = ld.max_stamp
			if shared is None:
				full = {'starid': np.asarray(catalog['starid']), 'tmag': np.asarray(catalog['tmag']),
					'column': (cat_px[i][:, 0] + c0).astype('float32'), 'row': (cat_px[i][:, 1] + r0).astype('float32')}
				cats.append(pipeline._catalog_of_stamp(full, ld.max_stamp))
			else:
				full = shared
				cats.append({k: v[offs_all[i]:offs_all[i + 1]] for k, v in cat_all.items()})
			hit = np.flatnonzero(tstar == starid[i]) if tstar is not None else ()
			if len(hit):
				k = int(hit[0])
				if tgt_px is not None:
					row, col = tgt_px[i][k, 1] + r0, tgt_px[i][k, 0] + c0
				else:
					row, col = targets['row'][k], targets['column'][k]
				pos[i] = float(row), float(col), float(targets['tmag'][k])
			else:
				k = first.get(int(starid[i])) if shared is not None else next(iter(np.flatnonzero(full['starid'] == starid[i])), None)
				if k is None:
					lost[i] = f"RuntimeError: Star could not be found in catalog: {int(starid[i]):d}"      # BasePhotometry.py:414
					pos[i] = 0.5 * (ld.max_stamp[0] + ld.max_stamp[1]), 0.5 * (ld.max_stamp[2] + ld.max_stamp[3]), 10.0
				else:
					pos[i] = float(full['row'][k]), float(full['column'][k]), float(full['tmag'][k])
		fr = pipeline.FramesResult(n)
		fr.stamp[:] = stamps_all
		apertures = [None] * n
		by_slot = [[None] * len(g) for g in groups]
		for i, (g, s) in enumerate(index):
			by_slot[g][s] = i
		if method == 'linpsf':
			return _linpsf_tpfs_chunk(ctx, fr, groups, by_slot, cats, pos, lost, starid, files, loaded, prf, linpsf_errors)   # (no K2P2 / extraction pass)
		for g, grp in enumerate(groups):
			ids = by_slot[g]
			offs =np.concatenate(([0], np.cumsum([len(cats[i]['starid']) for i in ids]))).astype('int64')
			cat = {k: np.concatenate([cats[i][k] for i in ids]) for k in ('starid', 'tmag', 'row', 'column', 'row_stamp', 'column_stamp')}
			scene = pipeline.GroupScene(grp.time, grp.quality, stamps_all[ids], offs, cat, pos[ids, 0], pos[ids, 1], pos[ids, 2],
				np.asarray(starid, dtype='int64')[ids], grp.aperture, cadence_s=grp.loaded[0].cadence or 1800)
			res = pipeline.run_aperture_group(ctx, scene, grp.cubes)
			res.update(cat_offsets=offs, cat_starid=cat['starid'], target_starid=scene.target_starid)
			fr.groups.append(res)
			for s, i in enumerate(ids):
				fr.group[i], fr.pos[i] = g, s
				apertures[i] = grp.aperture[s]
				if i in lost:
					fr.status[i], fr.errors[i] = STATUS.ERROR.value, [lost[i]]
					continue
				status, fr.has_result[i], messages = _one_attempt(res['flags'][s])
				fr.status[i] = status.value
				if messages:
					fr.errors[i] = messages
				if int(res['flags'][s]) >> 8 == 6:
					res['contamination'][s] = np.nan                    # photometry.py:243-246
		out = TpfBatchResults(fr, starid, pos[:, 2], files, loaded, apertures)
		if method != 'aperture':
			_halo_switch_tpfs(ctx, out, groups, by_slot, cats, pos, lost, method, settings)   # (while the cubes are resident)
	finally:
		for grp in groups:
			grp.free()
	return out


def _halo_switch_tpfs(ctx, out, groups, by_slot, cats, pos, lost, method, settings):
	"""The method switch of ``tessphot(None, ...)`` (tessphot.py:76-109) for a chunk of target pixel files after its aperture passes, or
	``tessphot('halo', ...)`` for every file (``method='halo'``): the chosen files of every group go through ``pipeline.halo_tpfs`` while
	the group's cubes are on the device.  With Halo photometry off a switch is recorded and the aperture result kept."""
	from . import pipeline, halo
	logger = logging.getLogger(__name__)
	if method == 'halo':
		idx = np.array([i for i in range(len(out)) if i not in lost], dtype='int64')
		out._halo_direct = True
	else:
		idx, codes = out.halo_switch(out.tmag, settings, datasource='tpf')
		for code in codes:
			logger.warning(_SWITCH_TEXT[int(code)])
		if len(idx) and not halo.enabled(settings):
			out.keep_aperture_results(idx, codes)
			return
	if len(idx) == 0:
		return
	chosen = set(int(i) for i in idx)
	parts, where = [], {}
	for g, grp in enumerate(groups):
		slots = [s for s, i in enumerate(by_slot[g]) if i in chosen]
		if not slots:
			continue
		ids = [by_slot[g][s] for s in slots]
		sums = np.stack([np.asarray(out.frames.groups[g]['sumimage'][s], dtype='float64') for s in slots])
		res = pipeline.halo_tpfs(ctx, grp, slots, [cats[i] for i in ids], pos[ids], starid=out.starid[ids], sumimage=sums, settings=settings)
		for j, i in enumerate(ids):
			where[i] = (len(parts), j)
		parts.append(res)
	out.switch_to_halo(idx, pipeline.HaloResultsOfGroups(parts, [where[int(i)] for i in idx]))


def tessphot_tpfs(ctx, files, catalog, targets=None, settings=None, output_folder=None, version=None, chunk_files=None, verify=True,
	workers=None, compresslevel=9, compress='zlib', table='host', method='aperture', prf=None):
	"""
	Aperture photometry of many target pixel files: what ``tessphot('aperture', starid, tpf.TpfStampSource(loaded, catalog,
	targets=targets), output_folder, datasource='tpf', version=version)`` returns and writes per file, with one pass of the fused
	kernel, one launch of the diagnostics and one download per group of files that share ``(H, W, T)``.  A generator: one
	:class:`TpfBatchResults` per chunk of ``chunk_files`` files, in input order.

	``method``: ``'aperture'`` (the default), ``None``, ``'halo'`` or ``'linpsf'`` -- what the per-file :func:`tessphot` does with it; anything
	else (``'psf'`` too) raises ``ValueError("Invalid method: '...'")`` before a file is opened.  ``None``: after a group's aperture pass the bright targets
	whose mask still carries flux on the stamp edge (``TpfBatchResults.halo_switch`` with the ``tpf`` datasource; every reason is logged
	as a warning) are redone with Halo photometry while the group's cubes are still on the device (``pipeline.halo_tpfs``: the problems
	built there by ``csrc/halo_cubes.hip``, one ``tp_halo_tvmin`` call per chunk of targets); ``results[i]`` then has ``method == 'halo'``,
	``halo_weightmap``, "Automatically switched to Halo photometry" among its errors and the aperture run's ``edge_flux``, and its file
	carries the ``WEIGHTMAP`` extension and the ``HALO_*`` cards.  With ``[halo] enabled`` off the aperture result is kept, the request
	recorded among its errors and OK turned into WARNING before the file is written, as the per-file entry does.  ``'halo'``: Halo
	photometry for every file (the aperture pass still runs: it supplies the sum images); ``NotImplementedError`` while Halo is off.
	``'linpsf'``: ``tessphot('linpsf', starid, TpfStampSource(loaded, catalog, prf=model), ...)`` for every file, one fit per group on the
	group's cubes as they lie (``pipeline.linpsf_tpfs``: the stars' positions formed on the device from every file's own ``POS_CORR``,
	``tp_star_positions_targets``).  No aperture pass runs: a result has no photometric mask, ``additional_headers`` ``PSF_CONT`` (and
	``PSF_FERR``), and the file's ``SUMIMAGE`` comes from ``tp_sumimage`` on the group's cube.  ``prf``: a ``psf.PRFModel``, a mapping
	``(camera, ccd) -> PRFModel``, or ``None`` for the SPOC model of each file's sector, camera and CCD under ``TESSPHOT_PSF_DIR``.
	``[linpsf] flux_errors`` of the settings is read once per call; while it is off every ``flux_err`` is NaN, as in the reference, and
	every target ends in ERROR "Final lightcurve errors are all NaNs" without a file, as the per-file call does.

	``files``: the paths; ``catalog`` / ``targets``: as for :class:`~photometry_amd.tpf.TpfStampSource` -- ``row`` / ``column`` in CCD
	pixels, or ``ra`` / ``dec``, which every file projects through the WCS of its own APERTURE header and moves by its stamp's place
	on the CCD (``tpf.project_for_files``: all files of a chunk in one call).  The stars of a stamp are those of the whole postage
	stamp plus the five-pixel buffer; the main target is the file's ``TICID``, or what a ``'file'`` column of ``targets`` names for the
	path (``tpf.main_targets``; list a file once per target).
	``chunk_files``: files per chunk; by default as many as keep the chunk's three cubes under a quarter (:data:`TPF_CHUNK_SHARE`) of
	the device memory that is free when the run starts, at most :data:`TPF_CHUNK_MAX` (:func:`tpf_chunk_files`).  The cubes of a chunk
	are freed before the next chunk is loaded.
	``output_folder`` with ``version``: the ``tess…-tasoc_lc.fits.gz`` of every OK / WARNING target is written on ``workers`` threads (at
	most 16) with gzip's ``compresslevel`` -- or, with ``compress='device'``, compressed on the device by the calling thread while the
	workers build the bytes and write the members (``lcfile.save_tpf_lightcurves``), and with ``table='device'`` besides, the tables' data
	units written on the device too (``ValueError`` without ``compress='device'``) --; ``QUALITY`` is all zero, what the plugin writes for a source without pixel flags.
	``verify``: the ``DATASUM`` check of ``tpf.load_tpfs``.
	With ``method='aperture'`` this is ``tessphot('aperture', ...)``: with ``[halo] enabled`` in the settings nothing is switched to Halo
	photometry, which is logged.
	"""
	from . import tpf, halo
	logger = logging.getLogger(__name__)
	if method is not None and method not in ('aperture', 'halo', 'linpsf'):
		raise ValueError(f"Invalid method: '{method}'")
	files = [str(f) for f in files]
	if not files:
		raise ValueError("tessphot_tpfs: no files")
	if output_folder is not None and version is None:
		raise ValueError("VERSION has not been set")
	if compress not in ('zlib', 'device'):
		raise ValueError(f"compress must be one of ('zlib', 'device'), not {compress!r}")
	from . import lcfile
	lcfile._check_table(table, compress)
	settings = load_settings() if settings is None else settings
	if method == 'halo' and not halo.enabled(settings):
		raise NotImplementedError("HaloPhotometry is off: set '[halo] enabled = true' in the settings file named by "
			"TESSPHOT_SETTINGS to run this engine's TV-min implementation")
	if method == 'aperture' and halo.enabled(settings):
		logger.info("Halo photometry is enabled in the settings, but batches of target pixel files do not switch methods: aperture results are kept.")
	linpsf_errors = method == 'linpsf' and LinPSFPhotometry.flux_errors(settings)      # ([linpsf] flux_errors: read once per call)
	headers = [tpf.read_tpf_header(f) for f in files]
	starid = tpf.main_targets(files, [h.header.get('TICID') for h in headers], targets)
	if chunk_files is None:
		chunk_files = tpf_chunk_files([h.aperture.shape + (h.table.n_rows,) for h in headers], ctx.mem_info()[0])
	chunk_files = max(1, int(chunk_files))
	for a in range(0, len(files), chunk_files):
		b = min(a + chunk_files, len(files))
		out = _tpf_chunk(ctx, files[a:b], headers[a:b], starid[a:b], catalog, targets, verify, method=method, settings=settings, prf=prf,
			linpsf_errors=linpsf_errors)
		out.ctx = ctx
		if output_folder is not None:
			out.save_lightcurves(output_folder, version, workers=workers, compresslevel=compresslevel, compress=compress, table=table)
		yield out
