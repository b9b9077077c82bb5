# -*- coding: utf-8 -*-
"""
Batched per-target pipelines over a stamp cube resident in HBM.

``run_aperture``: A1 sum image -> A2..A5b K2P2 masks + A7 contamination -> A6 extraction,
i.e. ``AperturePhotometry.do_photometry`` (photometry/AperturePhotometry/photometry.py:44-257)
for every target of the batch at once.
"""

import ctypes
import os
import numpy as np
from . import engine, _lib, wcs
from .engine import TESS_DEFAULT_BITMASK
from ._lib import TessphotError
from .device import DeviceCube, device_view
from .status import STATUS


class ApertureBatch(object):
	"""Device-resident inputs of a batch (cubes + per-target metadata)."""

	def __init__(self, ctx, scene, cubes='host'):
		self.ctx = ctx
		self.scene = scene
		# raw mode: the cubes hold the RAW flux; the background is estimated on the device (B*, B2) and
		# subtracted on the fly (B3) -- nothing but the raw + error cubes ever lives in HBM.
		self.raw_mode = False
		if isinstance(cubes, str) and cubes == 'host':
			self.images = DeviceCube.from_host(ctx, scene.images)
			self.images_err = DeviceCube.from_host(ctx, scene.images_err)
			self.backgrounds = DeviceCube.from_host(ctx, scene.backgrounds)
		elif isinstance(cubes, str) and cubes == 'host_aperture_only':
			# BASELINE configs[1]: images + errors, no background cube (flux_background comes out NaN)
			self.images = DeviceCube.from_host(ctx, scene.images)
			self.images_err = DeviceCube.from_host(ctx, scene.images_err)
			self.backgrounds = None
		elif isinstance(cubes, str) and cubes == 'host_raw':
			self.images = DeviceCube.from_host(ctx, scene.raw)
			self.images_err = DeviceCube.from_host(ctx, scene.raw_err)
			self.backgrounds = None
			self.raw_mode = True
		elif 'raw' in cubes:
			self.images, self.images_err, self.backgrounds = cubes['raw'], cubes.get('raw_err', cubes.get('images_err')), None
			self.raw_mode = True
		else:
			self.images, self.images_err, self.backgrounds = cubes['images'], cubes.get('images_err'), cubes.get('backgrounds')
		self.time_smooth = {1800: 3, 600: 9}.get(int(round(getattr(scene, 'cadence_s', 1800))), 3) # prepare.py:258
		self.n_targets = self.images.n_targets
		self.n_cad = self.images.n_cad
		self.height, self.width = self.images.height, self.images.width
		# the per-batch metadata -- quality flags, time stamps, stamps, the ragged catalogue and the target columns -- travel as ONE
		# host block and one upload (a batched entry builds a batch per stamp-size group and round: fifteen small uploads each were
		# a fifth of its time); the arrays below are views into that block
		c = scene.catalog
		fields = [('quality', np.asarray(scene.quality, dtype='int32')), ('time', np.asarray(scene.time, dtype='float64')),
			('stamps', np.asarray(scene.stamps, dtype='int32')), ('cat_offsets', np.asarray(scene.cat_offsets, dtype='int64')),
			('cat_starid', np.asarray(c['starid'], dtype='int64')), ('cat_tmag', np.asarray(c['tmag'], dtype='float32')),
			('cat_row', np.asarray(c['row'], dtype='float32')), ('cat_column', np.asarray(c['column'], dtype='float32')),
			('cat_row_stamp', np.asarray(c['row_stamp'], dtype='float32')), ('cat_column_stamp', np.asarray(c['column_stamp'], dtype='float32')),
			('target_pos_row', np.asarray(scene.target_pos_row, dtype='float64')), ('target_pos_column', np.asarray(scene.target_pos_column, dtype='float64')),
			('target_tmag', np.asarray(scene.target_tmag, dtype='float64')), ('target_starid', np.asarray(scene.target_starid, dtype='int64'))]
		offs, total = [], 0
		for _name, a in fields:
			offs.append(total)
			total = -(-(total + max(a.nbytes, 16)) // 256) * 256
		total = -(-total // 4) * 4
		if total <= (256 << 10):
			# small blocks: the library's ring of page-locked memory (tp_memcpy_h2d returns once the copy is queued)
			blob = np.zeros(total, dtype='uint8')
			for (_name, a), o in zip(fields, offs):
				blob[o:o + a.nbytes] = np.ascontiguousarray(a).view('uint8').ravel()
			self._meta = ctx.array(blob)
		else:
			# (page-locked, from the context's pool: the copy is queued and the host goes on -- a pageable block above 256 KB would wait for its DMA)
			self._meta_host = ctx.pinned_block(total)
			blob = self._meta_host.array
			for (_name, a), o in zip(fields, offs):
				blob[o:o + a.nbytes] = np.ascontiguousarray(a).view('uint8').ravel()
			self._meta = ctx.empty((total,), 'uint8')
			ctx._check(ctx.lib.tp_upload_cube_async(ctx.handle, self._meta.ptr, total // 4, self._meta_host.ptr, total // 4, 1, total // 4))
		for (name, a), o in zip(fields, offs):
			setattr(self, name, device_view(ctx, self._meta.ptr + o, a.shape, a.dtype, base=self._meta))
		ap = getattr(scene, 'aperture', None)
		if ap is None:
			# every pixel collected (bit 1 of BasePhotometry.aperture, BasePhotometry.py:1043; the kernels require a finite sum-image
			# pixel themselves): set on the device, 0x01010101 per pixel -- bit 1 is what the mask builder reads
			self.aperture = ctx.empty((self.n_targets, self.height, self.width), 'int32')
			self.aperture.fill_bytes(1)
		else:
			self.aperture = ctx.array(np.asarray(ap, dtype='int32'))

	def __del__(self):
		# the upload may still be in flight when the last reference goes: wait for the stream, then the block goes back to the pool
		h = self.__dict__.pop('_meta_host', None)
		if h is not None:
			try:
				self.ctx.sync()
				self.ctx.pinned_release(h)
			except Exception: # noqa: B902
				pass

	#: per-target arrays (sliced by :meth:`chunk`); the flat catalogue arrays are shared because the
	#: CSR offsets are absolute
	_PER_TARGET = ('images', 'images_err', 'backgrounds', 'stamps', 'target_pos_row', 'target_pos_column',
		'target_tmag', 'target_starid', 'aperture')

	def chunk(self, start, count):
		"""Non-owning view of the targets ``[start, start+count)`` (same HBM)."""
		v = ApertureBatch.__new__(ApertureBatch)
		v.__dict__.update(self.__dict__)
		v.__dict__.pop('_meta_host', None)   # the view does not own the upload's host block
		for name in self._PER_TARGET:
			a = getattr(self, name)
			setattr(v, name, None if a is None else a.slice0(start, count))
		v.cat_offsets = self.cat_offsets.slice0(start, count + 1)
		if len(self.quality.shape) == 2:
			v.quality = self.quality.slice0(start, count)
		v.n_targets = int(count)
		return v


class ApertureWork(object):
	"""
	Device-resident outputs / scratch of the aperture pipeline (allocated once, reused per step).

	``packed=True`` carves the per-target results a scheduler consumes -- the light-curve block ``[5][Nt][T]`` float64,
	``contamination`` float64, ``status`` / ``flags`` int32 and the ``mask`` uint8 (the output
	block of a rank), with ``psf=True`` also the LinPSF light curve, contamination and status -- out of ONE allocation
	(``self.block``, layout: ``comm.packed_block_layout``), so that the per-step gather of a multi-GPU run is a single message.
	"""

	def __init__(self, ctx, batch, packed=False, psf=False, capacity=None, cat_capacity=0, extras=False):
		"""``capacity`` >= the batch's targets lays the packed block out for that many (the padded shard size every rank of a
		sharded run sends); ``cat_capacity`` > 0 puts the catalogue flags ``cat_in_mask`` into the block as well."""
		from . import comm as tpcomm
		Nt, T, H, W = batch.n_targets, batch.n_cad, batch.height, batch.width
		self.sumimage = self.diagnostics = None
		self.block = None
		self.psf_flux = self.psf_contamination = self.psf_status = None
		n_cat = max(int(batch.scene.cat_offsets[-1]), 1)
		self.cat_in_mask = None
		if packed:
			cap = Nt if capacity is None else int(capacity)
			if cap < Nt or (cat_capacity and cat_capacity < n_cat):
				raise ValueError('block capacity below the size of the batch')
			layout, nbytes = tpcomm.packed_block_layout(cap, T, H, W, psf=psf, n_cat=int(cat_capacity), extras=extras)
			Nt = cap
			self.block = ctx.zeros((nbytes,), 'uint8')
			b = self.block
			view = lambda name: device_view(ctx, b.ptr + layout[name][0], layout[name][1], layout[name][2], base=b) # noqa: E731
			self.lc = engine.LightCurves(ctx, Nt, T, block=view('lc'))
			self.contamination, self.status, self.flags, self.mask = view('contamination'), view('status'), view('flags'), view('mask')
			if psf:
				self.psf_flux, self.psf_contamination, self.psf_status = view('psf_flux'), view('psf_contamination'), view('psf_status')
			if cat_capacity:
				self.cat_in_mask = view('cat_in_mask')
			if extras:   # (with a capacity above the batch the views cover the capacity: the kernels address the first Nt entries)
				self.sumimage, self.diagnostics = view('sumimage'), view('diagnostics')
			self.block_layout = layout
			Nt = batch.n_targets
		else:
			self.mask = ctx.zeros((Nt, H, W), 'uint8')
			self.status = ctx.zeros((Nt,), 'int32')
			self.flags = ctx.zeros((Nt,), 'int32')
			self.contamination = ctx.zeros((Nt,), 'float64')
			self.lc = engine.LightCurves(ctx, Nt, T)
		self.diag = ctx.zeros((Nt, 8), 'float64')
		if self.cat_in_mask is None:
			self.cat_in_mask = ctx.zeros((n_cat,), 'uint8')
		if self.sumimage is None:
			self.sumimage = ctx.empty((Nt, H, W), 'float64')
		if self.diagnostics is None:
			self.diagnostics = ctx.zeros((Nt, 10), 'float64')
		self.bkg_raw = self.bkg = None
		if batch.raw_mode:
			pitch = batch.images.t_pitch
			self.bkg_raw = ctx.zeros((Nt, pitch), 'float32')
			self.bkg = ctx.zeros((Nt, pitch), 'float32')

	def chunk(self, start, count):
		"""Non-owning view of the targets ``[start, start+count)`` (same HBM)."""
		v = ApertureWork.__new__(ApertureWork)
		v.__dict__.update(self.__dict__)
		for name in ('sumimage', 'mask', 'status', 'flags', 'contamination', 'diag', 'lc', 'diagnostics', 'bkg_raw', 'bkg'):
			a = getattr(self, name)
			setattr(v, name, None if a is None else a.slice0(start, count))
		return v


def aperture_step(ctx, batch, work, masks_from=None, fused=True):
	"""
	One pass of the aperture hot path over the batch; everything stays in HBM.

	``fused``: one launch with a wavefront per target (``tp_aperture_photometry``); ``False`` runs the three
	stand-alone kernels A1, K2P2, A6 back to back (bit-identical outputs).
	``masks_from``: optional ``(mask uint8 DeviceArray, status int32 DeviceArray)`` to bypass the
	on-device K2P2 (used by tests that inject the oracle's masks; implies the stand-alone kernels).
	"""
	subtract, backgrounds = None, batch.backgrounds
	if batch.raw_mode and fused and masks_from is None:
		# the raw cube is read ONCE: B*, B2 and the sum image of raw - background (A1 with B3 on the fly) in one pass,
		# then the mask and the extraction, which read in-mask pixel rows only
		engine.background_sumimage(ctx, batch.images, batch.quality, batch.time_smooth, bkg_raw=work.bkg_raw, bkg=work.bkg, sumimage=work.sumimage)
		engine.aperture_photometry(ctx, batch, work, subtract=work.bkg, backgrounds=work.bkg, sumimage_given=True)   # A2..A7
		return work
	if batch.raw_mode:
		engine.background_stamp(ctx, batch.images, out=work.bkg_raw)                           # B*
		engine.smooth_time(ctx, work.bkg_raw, batch.n_cad, batch.time_smooth, out=work.bkg)    # B2
		subtract = backgrounds = work.bkg                                                      # B3 on the fly
	if fused and masks_from is None:
		engine.aperture_photometry(ctx, batch, work, subtract=subtract, backgrounds=backgrounds)   # A1..A7
		return work
	engine.sumimage(ctx, batch.images, batch.quality, out=work.sumimage, subtract=subtract)    # A1
	if masks_from is None:
		engine.k2p2_masks(ctx, batch, work)                                                    # A2..A5b, A7
		mask, status = work.mask, work.status
	else:
		mask, status = masks_from
	engine.aperture_extract(ctx, batch.images, batch.images_err, backgrounds, mask, batch.stamps, status=status, out=work.lc,
		subtract=subtract)                                                                     # A6
	return work


def aperture_diagnostics(ctx, batch, work, status=None, mask=None):
	"""
	The light-curve diagnostics of the batch (BasePhotometry.py:1343-1407) from the device-resident outputs of
	:func:`aperture_step`; fills ``work.diagnostics`` ``(Nt, 10)`` (columns ``engine.DIAGNOSTICS_COLUMNS``).
	"""
	engine.lightcurve_diagnostics(ctx, work.lc, batch.time, batch.quality, status=work.status if status is None else status,
		sumimage=work.sumimage, mask=work.mask if mask is None else mask, out=work.diagnostics)
	return work.diagnostics


def run_aperture(ctx, scene, cubes='host', masks=None, diagnostics=True):
	"""
	Convenience: upload (or adopt device cubes), run one :func:`aperture_step`, download.

	Returns a dict of host arrays: ``sumimage, mask, status, flags, contamination, diag, cat_in_mask,
	flux, flux_err, flux_background, pos_centroid, diagnostics``.
	"""
	batch = ApertureBatch(ctx, scene, cubes=cubes)
	work = ApertureWork(ctx, batch)
	masks_from = None
	if masks is not None:
		m = ctx.array(np.asarray(masks, dtype='uint8'))
		st = ctx.array(np.ones(batch.n_targets, dtype='int32'))
		masks_from = (m, st)
	aperture_step(ctx, batch, work, masks_from=masks_from)
	if diagnostics and masks_from is None:
		aperture_diagnostics(ctx, batch, work)
	elif diagnostics:
		aperture_diagnostics(ctx, batch, work, status=masks_from[1], mask=masks_from[0])
	ctx.sync()
	out = work.lc.to_host()
	if diagnostics:
		out['diagnostics'] = work.diagnostics.to_host()
	out['sumimage'] = work.sumimage.to_host()
	if batch.raw_mode:
		out['background'] = work.bkg.to_host()[:, :batch.n_cad]
		out['background_raw'] = work.bkg_raw.to_host()[:, :batch.n_cad]
	if masks_from is None:
		out['mask'] = work.mask.to_host()
		out['status'] = work.status.to_host()
		out['flags'] = work.flags.to_host()
		out['contamination'] = work.contamination.to_host()
		out['diag'] = work.diag.to_host()
		out['cat_in_mask'] = work.cat_in_mask.to_host()
	else:
		out['mask'] = masks_from[0].to_host()
		out['status'] = masks_from[1].to_host()
	return out


class GroupScene(object):
	"""
	The ``Scene`` contract :class:`ApertureBatch` reads, for targets that share a stamp shape and a number of cadences and nothing
	else (the files of a ``tpf.TpfGroup``): ``quality`` and ``time`` ``(n, T)``, one row per target, ``stamps`` ``(n, 4)``, the ragged
	catalogue (``cat_offsets`` and ``catalog`` with ``starid, tmag, row, column, row_stamp, column_stamp``), the ``target_*`` columns and
	the per-target ``aperture`` ``(n, H, W)``.
	"""

	def __init__(self, time, quality, stamps, cat_offsets, catalog, target_pos_row, target_pos_column, target_tmag, target_starid, aperture, cadence_s=120):
		self.time = np.ascontiguousarray(time, dtype='float64')
		self.quality = np.ascontiguousarray(quality, dtype='int32')
		if self.time.ndim != 2 or self.quality.shape != self.time.shape:
			raise ValueError("GroupScene: time and quality are (targets, cadences)")
		self.n_targets, self.n_cad = self.time.shape
		self.stamps = np.asarray(stamps, dtype='int32').reshape(self.n_targets, 4)
		self.height, self.width = int(self.stamps[0, 1] - self.stamps[0, 0]), int(self.stamps[0, 3] - self.stamps[0, 2])
		self.cat_offsets = np.asarray(cat_offsets, dtype='int64')
		self.catalog = catalog
		self.target_pos_row, self.target_pos_column = np.asarray(target_pos_row, dtype='float64'), np.asarray(target_pos_column, dtype='float64')
		self.target_tmag, self.target_starid = np.asarray(target_tmag, dtype='float64'), np.asarray(target_starid, dtype='int64')
		self.aperture = np.asarray(aperture, dtype='int32')
		self.cadence_s = cadence_s

	def catalog_of(self, i):
		a, b = self.cat_offsets[i], self.cat_offsets[i + 1]
		return {k: v[a:b] for k, v in self.catalog.items()}


def run_aperture_group(ctx, scene, cubes):
	"""
	:func:`run_aperture` for a :class:`GroupScene` over device cubes as they are: one :class:`ApertureBatch`, one packed
	:class:`ApertureWork`, one :func:`aperture_step`, one :func:`aperture_diagnostics` with the per-target time vectors, and one
	download of the packed block.  Returns the dict of host arrays of :func:`run_aperture` (without ``diag``) and the light-curve block
	``lc`` ``(5, n, T)`` they are planes of, all views of that one download.
	"""
	batch = ApertureBatch(ctx, scene, cubes=cubes)
	if (batch.n_targets, batch.n_cad, batch.height, batch.width) != (scene.n_targets, scene.n_cad, scene.height, scene.width):
		raise ValueError("run_aperture_group: the cubes are not the scene's targets, cadences and stamp shape")
	n_cat = max(int(scene.cat_offsets[-1]), 1)
	work = ApertureWork(ctx, batch, packed=True, cat_capacity=n_cat, extras=True)
	aperture_step(ctx, batch, work)
	aperture_diagnostics(ctx, batch, work)
	blob = work.block.to_host()                                          # (waits for the stream)
	out = {}
	for name, (off, shape, dtype) in work.block_layout.items():
		out[name] = np.frombuffer(blob, dtype=dtype, count=int(np.prod(shape)), offset=off).reshape(shape)
	lc = out['lc']
	out['flux'], out['flux_err'], out['flux_background'] = lc[0], lc[1], lc[2]
	out['pos_centroid'] = np.stack((lc[3], lc[4]), axis=-1)
	return out


class LinPSFBatch(object):
	"""
	Device-resident inputs of the LinPSF pipeline (linpsf_photometry.py:79-219) for a batch:
	image cube, per-target spline tables (P1), fitted-star lists and their per-cadence positions
	(``catalog_attime``: reference position + jitter, host geometry).
	"""

	def __init__(self, ctx, scene, prf_model, images=None, subtract=None, work=None):
		"""``work``: an ``ApertureWork(packed=True, psf=True)`` whose block receives the light curve, contamination and status."""
		from . import psf as hpsf
		self.ctx, self.scene, self.model = ctx, scene, prf_model
		self.images = DeviceCube.from_host(ctx, scene.images) if images is None else images
		self.subtract = subtract
		sel, star_offsets, target_index = hpsf.select_stars(scene.catalog, scene.cat_offsets, scene.target_starid)
		self.sel, self.star_offsets_h, self.target_index_h = sel, star_offsets, target_index
		self.max_stars = int(np.diff(star_offsets).max()) if len(star_offsets) > 1 else 1
		rs = scene.catalog['row_stamp'][sel].astype('float64')
		cs = scene.catalog['column_stamp'][sel].astype('float64')
		T = scene.n_cad
		pitch = self.images.t_pitch
		pos_row = np.zeros((len(rs), pitch))
		pos_col = np.zeros((len(rs), pitch))
		pos_row[:, :T] = rs[:, None] + scene.jitter[None, :, 1]
		pos_col[:, :T] = cs[:, None] + scene.jitter[None, :, 0]
		self.pos_row, self.pos_col = ctx.array(pos_row), ctx.array(pos_col)
		self.star_offsets, self.target_index = ctx.array(star_offsets), ctx.array(target_index)
		self.base_coef = ctx.array(prf_model.base_coef)
		self.weights = ctx.array(prf_model.weights(scene.stamps))
		self.tx, self.ty = ctx.array(prf_model.tx), ctx.array(prf_model.ty)
		self.coef = ctx.empty((scene.n_targets, prf_model.base_coef.shape[1]), 'float64')
		self.out = self.result_for(work)
		self.n_fit_stars = len(rs)

	def result_for(self, work=None):
		"""Output arrays of the fit; the per-target results inside ``work``'s packed block when given."""
		n_fit = int(self.star_offsets_h[-1])
		if work is None or work.psf_flux is None:
			return engine.LinPSFResult(self.ctx, self.scene.n_targets, n_fit, self.scene.n_cad)
		return engine.LinPSFResult(self.ctx, self.scene.n_targets, n_fit, self.scene.n_cad, flux=work.psf_flux,
			contamination=work.psf_contamination, status=work.psf_status)


def linpsf_step(ctx, batch, cutoff_radius=5.0, out=None, subtract=None):
	"""One pass of the LinPSF hot path: P1 table blend, P2-P4 fit + contamination."""
	out = batch.out if out is None else out
	engine.linpsf_prf(ctx, batch.base_coef, batch.weights, out=batch.coef)
	engine.linpsf_fit(ctx, batch.images, batch.coef, batch.tx, batch.ty, batch.star_offsets, batch.target_index,
		batch.pos_row, batch.pos_col, batch.max_stars, cutoff_radius=cutoff_radius, subtract=batch.subtract if subtract is None else subtract, out=out)
	return out


#--------------------------------------------------------------------------------------------------
# Aperture photometry of many targets of one CCD region, INCLUDING the stamp-resize retries
#--------------------------------------------------------------------------------------------------
class FrameStack(object):
	"""
	The image groups of one CCD region resident in HBM -- what the reference keeps in its HDF5 file as ``images/%04d``,
	``images_err/%04d``, ``backgrounds/%04d`` (prepare.py:136-141) and reads back cut-out by cut-out for every target and every
	stamp resize (BasePhotometry.py:720-751).  ``frames``: dict of float32 host arrays ``(T, R, C)`` covering CCD rows
	``[row0, row0 + R)`` and columns ``[col0, col0 + C)`` (``row0 / col0`` = PIXEL_OFFSET_ROW / COLUMN of the file).
	"""

	def __init__(self, ctx, frames, row0, col0, sumimage=None):
		"""``frames``: host arrays (uploaded) or float32 DeviceArrays ``(T, R, C)`` already in HBM (e.g. from ``frameio.load_stack``).
		``sumimage`` (or ``frames['sumimage']``): the region's sum image, float64 ``(R, C)`` -- the HDF5 dataset ``sumimage`` of the
		reference's file (prepare.py:450-453, 459; ``prepare.prepare_frames`` returns it); without one it is formed from the image
		stack when a batch first needs it (:meth:`sumimage_for`).  Optionally ``frames['pixel_flags']``, uint8 ``(T, R, C)`` (host array or
		DeviceArray, as ``prepare.prepare_frames`` returns it), and ``frames['backgrounds_pixels_used']``, ``(R, C)``: kept for the
		light-curve files (``BatchResults.save_lightcurves``), read by nothing else."""
		from .device import DeviceArray
		self.ctx = ctx
		self.row0, self.col0 = int(row0), int(col0)
		self.names = ('images', 'images_err', 'backgrounds')
		self.dev = {k: (frames[k] if isinstance(frames[k], DeviceArray) else ctx.array(np.ascontiguousarray(frames[k], dtype='float32'))) for k in self.names}
		self.n_cad, self.n_rows, self.n_cols = self.dev['images'].shape
		self.limits = (self.row0, self.row0 + self.n_rows, self.col0, self.col0 + self.n_cols)
		if sumimage is None and hasattr(frames, 'get'):
			sumimage = frames.get('sumimage')
		self._sumimage = self._sumimage_key = None
		self._time_major = None
		if sumimage is not None:
			self._sumimage = sumimage if isinstance(sumimage, DeviceArray) else ctx.array(np.ascontiguousarray(sumimage, dtype='float64'))
			if tuple(self._sumimage.shape) != (self.n_rows, self.n_cols):
				raise ValueError('the sum image must have the shape of a frame')
			self._sumimage_key = 'given'
			ctx.sync()
		#: the pixel flags of the prepare stage, uint8 DeviceArray ``(T, R, C)`` (``pixel_flags/%04d`` of the reference's file), or None:
		#: only the light-curve files read them (:meth:`stamp_flag_series`); they live and go with the stack
		self.pixel_flags = None
		#: ``backgrounds_pixels_used`` of the prepare stage, bool host image ``(R, C)``, or None (bit 4 of the files' APERTURE images)
		self.backgrounds_pixels_used = None
		if hasattr(frames, 'get'):
			flags, used = frames.get('pixel_flags'), frames.get('backgrounds_pixels_used')
			if flags is not None:
				self.pixel_flags = flags if isinstance(flags, DeviceArray) else ctx.array(np.ascontiguousarray(flags, dtype='uint8'))
				if tuple(self.pixel_flags.shape) != (self.n_cad, self.n_rows, self.n_cols) or self.pixel_flags.dtype != np.uint8:
					raise ValueError('the pixel flags must be uint8 with the shape of the image stack')
			if used is not None:
				used = used.to_host() if isinstance(used, DeviceArray) else np.asarray(used)
				if used.shape != (self.n_rows, self.n_cols):
					raise ValueError('backgrounds_pixels_used must have the shape of a frame')
				self.backgrounds_pixels_used = used.astype(bool)

	def stamp_flag_series(self, stamps, flag_mask, out_value):
		"""
		``(N, T)`` int32 on the host: ``out_value`` where any pixel of stamp ``stamps[i]`` (``(r1, r2, c1, c2)`` in CCD pixels; all -1: no
		stamp) carries a bit of ``flag_mask`` in frame ``t``, else 0 -- ``np.any(pixelflags_cube & flag_mask != 0, axis=(0, 1))`` of
		save_lightcurve (BasePhotometry.py:1445-1449) for a whole batch: one launch (``tp_stamp_flag_series``), one download.  All zero
		for a stack without pixel flags, as for a source without them (``BasePhotometry.pixelflags_cube``).
		"""
		st = np.ascontiguousarray(stamps, dtype='int64').reshape(-1, 4)
		if self.pixel_flags is None or len(st) == 0:
			return np.zeros((len(st), self.n_cad), dtype='int32')
		ctx = self.ctx
		out = ctx.empty((len(st), self.n_cad), 'int32')
		ctx._check(ctx.lib.tp_stamp_flag_series(ctx.handle, self.pixel_flags.ptr, self.n_cad, self.n_rows, self.n_cols, self.n_rows * self.n_cols, self.row0, self.col0,
			len(st), st.ctypes.data, int(flag_mask), int(out_value), out.ptr, self.n_cad))
		host = out.to_host()
		out.free()
		return host

	def sumimage_for(self, quality):
		"""
		The sum image of the region, float64 DeviceArray ``(R, C)``: the mean of the finite pixels of the frames with good quality
		(prepare.py:450-453, 459).  For an FFI target the reference crops it (``BasePhotometry.sumimage``, BasePhotometry.py:1001-1006)
		-- no sum over a stamp's own cube -- and so do the passes of :func:`aperture_frames`.  Given with the stack, or formed once per
		quality series (``tp_frames_sumimage``: the float64 sums in cadence order, as prepare.py accumulates them).
		"""
		if self._sumimage_key == 'given':
			return self._sumimage
		q = np.ascontiguousarray(quality, dtype='int32')
		key = q.tobytes()
		if self._sumimage_key != key:
			# (a NEW array per quality series: jobs in flight may still read the one of the series before; they keep it alive)
			ctx = self.ctx
			sumimage = ctx.empty((self.n_rows, self.n_cols), 'float64')
			dq = ctx.array(q)
			ctx._check(ctx.lib.tp_frames_sumimage(ctx.handle, self.n_cad, self.n_rows * self.n_cols, self.n_rows * self.n_cols, self.dev['images'].ptr, dq.ptr,
				int(TESS_DEFAULT_BITMASK), sumimage.ptr))
			ctx.sync()      # other streams (the jobs' contexts) read it
			dq.free()
			self._sumimage, self._sumimage_key = sumimage, key
		return self._sumimage

	def time_major(self):
		"""
		The three stacks once more, TIME-MAJOR: float32 DeviceArrays ``(R * C, t_pitch)`` (``tp_frames_transpose``; formed on first use,
		kept with the stack), or ``None`` when ``TESSPHOT_FRAMES_TIME_MAJOR=0`` or the device has no room for them.  With them the
		native engine cuts nothing: a mask pixel's time series is one row of the stack (``tp_aperture_extract_stack``), where every
		batch of targets used to cut the in-mask rows out of all frames again -- the reference's ``_load_cube`` per target and per stamp
		resize (BasePhotometry.py:720-751).  Costs the stacks' size a second time in HBM, and one pass over them per region.
		"""
		if self._time_major is False or os.environ.get('TESSPHOT_FRAMES_TIME_MAJOR', '1') == '0':
			return None
		if self._time_major is None:
			ctx = self.ctx
			t_pitch = (self.n_cad + 31) // 32 * 32
			npix = self.n_rows * self.n_cols
			out = {}
			try:
				for k in self.names:
					out[k] = ctx.empty((npix, t_pitch), 'float32')
					ctx._check(ctx.lib.tp_frames_transpose(ctx.handle, self.dev[k].ptr, self.n_cad, npix, npix, out[k].ptr, t_pitch))
				ctx.sync()      # other streams (the jobs' contexts) read them
			except TessphotError:
				for a in out.values():
					a.free()
				self._time_major = False
				return None
			self._time_major = (out, t_pitch)
		return self._time_major


def _catalog_of_stamp(catalog, stamp, buffer_size=5):
	"""Stars inside the stamp plus its 5-pixel buffer with the float32 stamp coordinates of BasePhotometry.catalog
	(BasePhotometry.py:1094-1181); the same selection as ``source.MemoryStampSource.catalog_in_stamp``."""
	r1, r2, c1, c2 = stamp
	row, col = catalog['row'], catalog['column']
	sel = (row >= r1 - 0.5 - buffer_size) & (row < r2 - 0.5 + buffer_size) & (col >= c1 - 0.5 - buffer_size) & (col < c2 - 0.5 + buffer_size)
	col64, row64 = np.asarray(col[sel], dtype='float64'), np.asarray(row[sel], dtype='float64')
	return {'starid': np.asarray(catalog['starid'][sel], dtype='int64'), 'tmag': np.asarray(catalog['tmag'][sel], dtype='float32'),
		'column': col64.astype('float32'), 'row': row64.astype('float32'),
		'column_stamp': (col64 - c1).astype('float32'), 'row_stamp': (row64 - r1).astype('float32')}


class _CatalogIndex(object):
	"""The catalogue of a CCD region binned into cells of ``cell`` x ``cell`` pixels (stars sorted by cell), for
	:func:`_catalogs_of_stamps`: the candidates of a stamp are the stars of the few cells it overlaps -- a row-sorted catalogue
	alone hands every stamp all the stars of its band of rows, hundreds of candidates for the handful that are kept."""
	def __init__(self, catalog, cell=16):
		self.catalog = catalog
		self.cell = int(cell)
		row = np.asarray(catalog['row'], dtype='float64')
		col = np.asarray(catalog['column'], dtype='float64')
		if len(row):
			self.r0 = int(np.floor(np.nanmin(row))) if np.isfinite(row).any() else 0
			self.c0 = int(np.floor(np.nanmin(col))) if np.isfinite(col).any() else 0
			finite = np.isfinite(row) & np.isfinite(col)
			cr = np.where(finite, np.floor((row - self.r0) / self.cell), 0).astype('int64')
			cc = np.where(finite, np.floor((col - self.c0) / self.cell), 0).astype('int64')
			self.n_cr, self.n_cc = int(cr.max()) + 1, int(cc.max()) + 1
			cid = np.where(finite, cr * self.n_cc + cc, self.n_cr * self.n_cc)   # stars without a position: a cell no stamp asks for
		else:
			self.r0 = self.c0 = 0
			self.n_cr = self.n_cc = 1
			cid = np.zeros(0, dtype='int64')
		self.order = np.argsort(cid, kind='stable')
		self.cell_start = np.searchsorted(cid[self.order], np.arange(self.n_cr * self.n_cc + 1), side='left')


def _catalogs_of_stamps(index, stamps, buffer_size=5):
	"""
	:func:`_catalog_of_stamp` for all stamps of a group at once, in CSR form: ``(offsets int64 [n + 1], dict of concatenated
	arrays)``; the stars of a stamp keep their catalogue order.  Candidate stars come from the cells of the binned catalogue the
	stamp (plus its buffer) overlaps, one contiguous run of the cell-sorted catalogue per row of cells; the row / column tests and the
	float32 stamp coordinates are the expressions of the per-stamp function evaluated on arrays.
	"""
	cat = index.catalog
	st = np.asarray(stamps, dtype='int64').reshape(-1, 4)
	n = len(st)
	B = index.cell
	rlo, rhi = st[:, 0] - 0.5 - buffer_size, st[:, 1] - 0.5 + buffer_size      # row >= rlo, row < rhi
	clo, chi = st[:, 2] - 0.5 - buffer_size, st[:, 3] - 0.5 + buffer_size
	cr0 = np.clip(np.floor((rlo - index.r0) / B).astype('int64'), 0, index.n_cr - 1)
	cr1 = np.clip(np.floor((rhi - index.r0) / B).astype('int64'), -1, index.n_cr - 1)
	cc0 = np.clip(np.floor((clo - index.c0) / B).astype('int64'), 0, index.n_cc - 1)
	cc1 = np.clip(np.floor((chi - index.c0) / B).astype('int64'), -1, index.n_cc - 1)
	# one run [cell_start[first cell], cell_start[last cell + 1]) per (stamp, row of cells)
	nrows = np.maximum(cr1 - cr0 + 1, 0) * (cc1 >= cc0)
	run_stamp = np.repeat(np.arange(n), nrows)
	run_row = np.arange(int(nrows.sum())) - np.repeat(np.cumsum(nrows) - nrows, nrows) + np.repeat(cr0, nrows)
	a = index.cell_start[run_row * index.n_cc + cc0[run_stamp]]
	b = index.cell_start[run_row * index.n_cc + cc1[run_stamp] + 1]
	cnt = b - a
	which = np.repeat(run_stamp, cnt)
	pos = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(a, cnt)
	star = index.order[pos]
	col, row = np.asarray(cat['column'])[star], np.asarray(cat['row'])[star]
	keep = (row >= rlo[which]) & (row < rhi[which]) & (col >= clo[which]) & (col < chi[which])
	which, star = which[keep], star[keep]
	o = np.argsort(which * (len(index.order) + 1) + star, kind='stable')   # catalogue order inside every stamp
	which, star = which[o], star[o]
	offsets = np.concatenate(([0], np.cumsum(np.bincount(which, minlength=n)))).astype('int64')
	col64, row64 = np.asarray(cat['column'], dtype='float64')[star], np.asarray(cat['row'], dtype='float64')[star]
	arrays = {'starid': np.asarray(cat['starid'], dtype='int64')[star], 'tmag': np.asarray(cat['tmag'], dtype='float32')[star],
		'column': col64.astype('float32'), 'row': row64.astype('float32'),
		'column_stamp': (col64 - st[which, 2]).astype('float32'), 'row_stamp': (row64 - st[which, 0]).astype('float32')}
	return offsets, arrays


class _RawBlock(object):
	"""``nbytes`` bytes at ``address`` through the array interface (no ctypes array type per size)."""
	__slots__ = ('__array_interface__',)

	def __init__(self, address, nbytes):
		self.__array_interface__ = {'shape': (int(nbytes),), 'typestr': '|u1', 'data': (int(address), True), 'version': 3}


def _view_bytes(address, nbytes):
	"""Read-only uint8 view of host memory owned by the library (a job's page-locked block: alive until the job is released)."""
	return np.asarray(_RawBlock(address, nbytes))


class FramesResult(object):
	"""
	Columnar result of :func:`aperture_frames`: one entry per target in arrays (``status``, ``stamp``, ``stamp_resizes``, ``has_result``),
	the rare per-target extras (log messages, ``edge_flux``) in sparse dicts, and the arrays the device passes returned kept group by
	group (a group = the targets of one pass that share a stamp size): target ``i`` is row ``pos[i]`` of group ``group[i]``.  Nothing is
	allocated per target until a per-target view is asked for: ``result[i]`` builds the dict the list-based API used to return.
	"""

	def __init__(self, n):
		self.n = int(n)
		self.status = np.zeros(n, dtype='int32')
		self.stamp = np.full((n, 4), -1, dtype='int64')
		self.stamp_resizes = np.zeros(n, dtype='int32')
		self.has_result = np.zeros(n, dtype=bool)
		self.group = np.full(n, -1, dtype='int32')
		self.pos = np.zeros(n, dtype='int32')
		self.errors = {}       # target -> list of "LEVEL: message" strings (targets without messages have no entry)
		self.edge_flux = {}    # target -> flux on the stuck edges (haloswitch quick break)
		#: per device pass: dict of host arrays.  They are READ-ONLY VIEWS of the page-locked block the pass was downloaded into and
		#: live as long as this result: :meth:`release` (and the result's deletion) hands the blocks to the next job's download.  Copy
		#: what has to outlive the result (``result[i]`` does: the per-target dict holds copies).
		self.groups = []
		self._job = None       # the native job (pipeline.FramesEngine) whose page-locked blocks the group arrays view

	def release(self):
		"""Give the page-locked blocks behind the group arrays back to their pool: the group arrays must not be used afterwards
		(they are dropped from ``groups``; a view a caller kept would read the next job's data)."""
		self.groups = []
		job, self._job = self._job, None
		if job is not None:
			job.release()

	def __del__(self):
		try:
			self.release()
		except Exception: # noqa: B902
			pass

	def __len__(self):
		return self.n

	def column(self, name, fill=np.nan):
		"""A per-target column gathered from the groups (``contamination``, ``mask_size``, or a ``DIAGNOSTICS_COLUMNS`` name)."""
		out = np.full(self.n, fill, dtype='float64')
		for g, grp in enumerate(self.groups):
			sel = np.flatnonzero(self.has_result & (self.group == g))
			if len(sel) == 0:
				continue
			rows = self.pos[sel]
			if name == 'contamination':
				out[sel] = grp['contamination'][rows]
			elif name == 'mask_size':
				out[sel] = grp['mask'][rows].reshape(len(rows), -1).sum(axis=1)
			else:
				out[sel] = grp['diagnostics'][rows, engine.DIAGNOSTICS_COLUMNS.index(name)]
		return out

	def __getitem__(self, i):
		i = int(i)
		if i < 0:
			i += self.n
		if not 0 <= i < self.n:
			raise IndexError(i)
		d = {'status': int(self.status[i]), 'errors': list(self.errors.get(i, ())), 'stamp_resizes': int(self.stamp_resizes[i])}
		if self.stamp[i, 1] >= 0:
			d['stamp'] = tuple(int(v) for v in self.stamp[i])
		if i in self.edge_flux:
			d['edge_flux'] = self.edge_flux[i]
		if self.has_result[i]:
			grp, j = self.groups[self.group[i]], int(self.pos[i])
			a, b = grp['cat_offsets'][j], grp['cat_offsets'][j + 1]
			inside = grp['cat_in_mask'][a:b].astype(bool)
			lc = grp['lc']   # the light-curve block (5, m, T): flux, flux_err, flux_background, centroid column, centroid row
			# (copies: the group arrays live in page-locked memory that goes back to the context's pool with this result)
			d.update(mask=grp['mask'][j].astype(bool), sumimage=np.array(grp['sumimage'][j]), flux=np.array(lc[0][j]), flux_err=np.array(lc[1][j]),
				flux_background=np.array(lc[2][j]), pos_centroid=np.stack((lc[3][j], lc[4][j]), axis=-1),   # (T, 2): column then row (BasePhotometry.py:428)
				contamination=float(grp['contamination'][j]),
				skip_targets=[int(s) for s in grp['cat_starid'][a:b][inside] if s != grp['target_starid'][j]],
				diagnostics=dict(zip(engine.DIAGNOSTICS_COLUMNS, grp['diagnostics'][j])))
		return d

	def __iter__(self):
		return (self[i] for i in range(self.n))


#: what the native engine reports as codes (csrc/frames.cpp) in the words of the reference's plugin
_EVENT_TEXT = {1: 'ERROR: No flux above threshold.', 2: 'WARNING: No masks found. Using minimum aperture.',
	3: 'WARNING: No mask found for main target. Using minimum aperture.', 4: 'ERROR: Too many masks.',
	6: 'WARNING: Could not resize stamp any further.', 7: 'ERROR: Stamp resize hit limit. Haloswitch quick break.',
	8: 'ERROR: Too many stamp resizes.', 9: 'ERROR: No targets in mask.', 12: 'ValueError: Invalid stamp selected'}


class _NativeCatalog(object):
	"""The catalogue of a region inside the library (``tp_frames_catalog``: copied and binned into cells once)."""
	def __init__(self, lib, catalog):
		self.lib = lib
		sid = np.ascontiguousarray(catalog['starid'], dtype='int64')
		tm = np.ascontiguousarray(catalog['tmag'], dtype='float32')
		row = np.ascontiguousarray(catalog['row'], dtype='float64')
		col = np.ascontiguousarray(catalog['column'], dtype='float64')
		h = ctypes.c_void_p()
		rc = lib.tp_frames_catalog_create(len(sid), sid.ctypes.data, tm.ctypes.data, row.ctypes.data, col.ctypes.data, ctypes.byref(h))
		if rc != 0:
			raise TessphotError(rc, (lib.tp_last_error(None) or b'').decode())
		self.handle = h.value

	def __del__(self):
		h, self.handle = getattr(self, 'handle', None), None
		if h:
			self.lib.tp_frames_catalog_destroy(h)


class FramesJob(object):
	"""A batch in flight in the native engine: :meth:`collect` waits for it and returns its :class:`FramesResult`."""
	def __init__(self, engine, handle, n, T, keep):
		self.engine, self.handle, self.n, self.T = engine, handle, int(n), int(T)
		self._keep = keep      # the stack and the catalogue: alive while the job runs

	def release(self):
		h, self.handle = self.handle, None
		if h and self.engine.handle:
			self.engine.lib.tp_frames_release(h)

	def __del__(self):
		try:
			self.release()
		except Exception: # noqa: B902
			pass

	def done(self):
		"""Has the job's worker finished (:meth:`collect` would not wait)?"""
		d = ctypes.c_int32(0)
		self.engine.lib.tp_frames_poll(self.handle, ctypes.byref(d))
		return bool(d.value)

	def collect(self):
		from . import comm as tpcomm
		lib, h, n, T = self.engine.lib, self.handle, self.n, self.T
		rc = lib.tp_frames_wait(h)
		if rc != 0:
			msg = (lib.tp_last_error(None) or b'').decode()
			self.release()
			raise TessphotError(rc, msg)
		self._keep = None
		out = FramesResult(n)
		out._job = self
		ng, ne = ctypes.c_int32(), ctypes.c_int64()
		lib.tp_frames_counts(h, ctypes.byref(ng), ctypes.byref(ne))
		has = np.zeros(n, dtype='uint8')
		lib.tp_frames_targets(h, out.status.ctypes.data, out.stamp.ctypes.data, out.stamp_resizes.ctypes.data, has.ctypes.data,
			out.group.ctypes.data, out.pos.ctypes.data)
		out.has_result = has.astype(bool)
		for g in range(ng.value):
			m, H, W, cap, ncat, blk, nb = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_void_p(), ctypes.c_uint64()
			lib.tp_frames_group(h, g, ctypes.byref(m), ctypes.byref(H), ctypes.byref(W), ctypes.byref(cap), ctypes.byref(ncat), ctypes.byref(blk), ctypes.byref(nb))
			# the fields of the packed block (comm.frames_block_fields: comm.packed_block_layout with the catalogue flags and the extras,
			# written out), as read-only views of the page-locked block -- this loop is the host's share of a batch (it was 1.0 ms of a
			# 7.7 ms call through packed_block_layout / unpack_block and one ctypes array TYPE per block size)
			mm, cc = m.value, cap.value
			host = _view_bytes(blk.value, nb.value)
			grp, off = {}, 0
			for name, shape, dtype, size in tpcomm.frames_block_fields(mm, T, H.value, W.value, cc):
				grp[name] = host[off:off + size].view(dtype).reshape(shape)
				off = -(-(off + size) // 256) * 256
			if off != nb.value:
				raise RuntimeError('the packed block of the native engine does not have the layout of comm.packed_block_layout')
			offs = np.empty(mm + 1, dtype='int64')
			cat_ids = np.empty(max(ncat.value, 0), dtype='int64')
			tids = np.empty(mm, dtype='int64')
			lib.tp_frames_group_lists(h, g, offs.ctypes.data, cat_ids.ctypes.data, tids.ctypes.data)
			grp.update(cat_offsets=offs, cat_starid=cat_ids, target_starid=tids)
			out.groups.append(grp)
		if ne.value:
			k = ne.value
			tgt, code, a, b, txt = (np.empty(k, dtype='int32') for _ in range(5))
			val = np.empty(k, dtype='float64')
			lib.tp_frames_events(h, tgt.ctypes.data, code.ctypes.data, a.ctypes.data, b.ctypes.data, val.ctypes.data, txt.ctypes.data)
			from .plugins import _MASK_EXCEPTIONS
			for e in range(k):
				i, c = int(tgt[e]), int(code[e])
				if c == 5:
					msg = 'RuntimeError: ' + _MASK_EXCEPTIONS[int(a[e])]
				elif c == 10:
					msg = 'ERROR: Device pass failed for a %dx%d stamp: %s' % (a[e], b[e], lib.tp_frames_text(h, int(txt[e])).decode())
				elif c == 11:
					msg = 'ERROR: Device pass failed while the light curves were copied: ' + lib.tp_frames_text(h, int(txt[e])).decode()
				else:
					msg = _EVENT_TEXT[c]
				out.errors.setdefault(i, []).append(msg)
				if c == 7:
					out.edge_flux[i] = float(val[e])
		return out


class FramesEngine(object):
	"""
	The native job engine of the batched drop-in entry (``tp_frames_*``, ``csrc/frames.cpp``): ``slots`` jobs in flight, each
	driven by a worker thread of the library on three streams of its own.  ``submit`` copies the batch's host arrays and
	returns at once; ``FramesJob.collect`` waits.  One engine per context (:meth:`of`), closed with it.
	"""
	def __init__(self, ctx, slots=4):
		self.ctx, self.lib, self.slots = ctx, ctx.lib, int(slots)
		h = ctypes.c_void_p()
		rc = self.lib.tp_frames_engine_create(ctx.device, self.slots, ctypes.byref(h))
		if rc != 0:
			raise TessphotError(rc, (self.lib.tp_last_error(None) or b'').decode())
		self.handle = h.value
		hbm = ctypes.c_uint64()
		self.lib.tp_frames_engine_info(self.handle, None, None, ctypes.byref(hbm))
		self.hbm_bytes = hbm.value

	#: jobs in flight the engine of a context is made for -- the most that pays (five measure the same as four, and every slot is five
	#: streams of the process's two dozen hardware queues; aperture_frames_pipelined clamps to it); the engine
	#: is made ONCE with all of them: remaking it for more slots would strand the jobs and results that point at the old one
	MAX_SLOTS = 4

	@classmethod
	def of(cls, ctx, slots=4):
		"""The engine of ``ctx`` (made on first use with :attr:`MAX_SLOTS` slots and kept until the context closes)."""
		if slots > cls.MAX_SLOTS:
			raise ValueError('the frames engine has %d slots' % cls.MAX_SLOTS)
		eng = ctx.__dict__.get('_frames_engine')
		if eng is None or eng.handle is None:
			eng = ctx.__dict__['_frames_engine'] = cls(ctx, slots=cls.MAX_SLOTS)
		return eng

	def catalog(self, catalog):
		"""The catalogue of a region copied into the library and binned (once per run over the region: the pipelined entry)."""
		return _NativeCatalog(self.lib, catalog)

	def submit(self, stack, targets, catalog, time, quality, settings=None, datasource='ffi', budget_share=1.0):
		from . import stamps as st
		from .plugins import load_settings, mag2flux
		settings = load_settings() if settings is None else settings
		tmag_limit = settings.getfloat('haloswitch', 'tmag_limit')
		flux_limit = settings.getfloat('haloswitch', 'flux_limit')
		sid = np.ascontiguousarray(targets['starid'], dtype='int64')
		tm = np.ascontiguousarray(targets['tmag'], dtype='float64')
		row = np.ascontiguousarray(targets['row'], dtype='float64')
		col = np.ascontiguousarray(targets['column'], dtype='float64')
		n = len(sid)
		first, valid = st.default_stamps(row, col, tm, stack.limits)
		first = np.ascontiguousarray(first, dtype='int64')
		valid8 = np.ascontiguousarray(valid, dtype='uint8')
		attempts = np.where(tm < 6, 10, 5).astype('int32')                    # photometry.py:70-73 (stamps.retry_limit)
		bright = (tm <= tmag_limit) & (not datasource.startswith('tpf:'))      # photometry.py:146
		budget_flux = np.where(bright, flux_limit * mag2flux(tm), np.nan).astype('float64')
		t = np.ascontiguousarray(time, dtype='float64')
		q = np.ascontiguousarray(quality, dtype='int32')
		if len(t) != stack.n_cad or len(q) != stack.n_cad:
			raise ValueError('time and quality must have one entry per frame of the stack')
		# an FFI target's sum image is a crop of the region's (BasePhotometry.py:1001-1006); a postage-stamp target ('tpf:...') sums its
		# own stamp (:1007-1019): no region sum image is handed over and every pass forms the stamps' own (tp_sumimage)
		sumimage = None if datasource.startswith('tpf:') else stack.sumimage_for(q)
		tm_stacks = None if sumimage is None else stack.time_major()
		sdesc = _lib.tp_frames_stack(stack.dev['images'].ptr, stack.dev['images_err'].ptr, stack.dev['backgrounds'].ptr,
			stack.n_cad, stack.n_rows, stack.n_cols, stack.row0, stack.col0, None if sumimage is None else sumimage.ptr,
			None if tm_stacks is None else tm_stacks[0]['images'].ptr, None if tm_stacks is None else tm_stacks[0]['images_err'].ptr,
			None if tm_stacks is None else tm_stacks[0]['backgrounds'].ptr, 0 if tm_stacks is None else tm_stacks[1])
		budget = float(os.environ.get('TESSPHOT_FRAMES_BUDGET_GB', 0)) * 1e9 or self.hbm_bytes / 4.0
		h = ctypes.c_void_p()
		rc = self.lib.tp_frames_submit(self.handle, ctypes.byref(sdesc), catalog.handle, n, sid.ctypes.data, tm.ctypes.data, row.ctypes.data, col.ctypes.data,
			first.ctypes.data, valid8.ctypes.data, attempts.ctypes.data, budget_flux.ctypes.data, t.ctypes.data, q.ctypes.data, budget * budget_share, ctypes.byref(h))
		if rc != 0:
			raise TessphotError(rc, (self.lib.tp_last_error(None) or b'').decode())
		return FramesJob(self, h.value, n, stack.n_cad, (stack, catalog, sumimage))

	def close(self):
		h, self.handle = self.handle, None
		if h:
			self.lib.tp_frames_engine_destroy(h)


def aperture_frames(ctx, stack, targets, catalog, time, quality, settings=None, datasource='ffi'):
	"""
	``AperturePhotometry.do_photometry`` INCLUDING its stamp-resize loop (photometry.py:75-170) for every target of a CCD region
	held in a :class:`FrameStack`: round after round, the targets still in play are grouped by stamp size, their stamps are cut
	out of the frames on the device, one fused pass per group produces sum image, mask and light curve, and the edge flags
	decide -- with the plugin's own rules (:mod:`photometry_amd.stamps`) -- who is finished, who gets a bigger stamp, and who
	gives up ("Too many stamp resizes." / "Stamp resize hit limit. Haloswitch quick break.").

	``targets``: dict of arrays ``starid, tmag, row, column`` (CCD positions, float64); ``catalog``: the same columns for every
	star of the region.  Returns a :class:`FramesResult` (columnar; ``result[i]`` is the per-target dict: ``status, stamp,
	stamp_resizes, errors`` and, unless the target ended in an error before the extraction, ``mask, sumimage, flux, flux_err,
	flux_background, pos_centroid, contamination, skip_targets, diagnostics``).  The common case -- the mask does not touch an
	edge and nothing is logged -- is decided for a whole group with array operations; only the targets that resize, warn or fail
	take the per-target path.  The rounds are driven by a worker thread of the library (``csrc/frames.cpp``, :class:`FramesEngine`):
	the host submits the batch and collects it.
	"""
	eng = FramesEngine.of(ctx)
	return eng.submit(stack, targets, eng.catalog(catalog), time, quality, settings=settings, datasource=datasource).collect()


def aperture_frames_pipelined(ctx, stack, batches, catalog, time, quality, settings=None, datasource='ffi', in_flight=4):
	"""
	:func:`aperture_frames` over consecutive batches of targets of one CCD region (``batches``: an iterable of ``targets`` dicts),
	``in_flight`` of them at a time, each on its own streams: the rounds of a batch are a strict chain -- queue the passes, wait,
	decide, queue the next round -- whose later links are a few latency-bound passes over the resized stamps that leave most of
	the chip idle, so the first round of the next batch runs under them and the host decides one batch while the device works on
	the other.  Yields one :class:`FramesResult` per batch, in order; every batch gives what a call of its own would.
	Every batch is a job of :class:`FramesEngine`: submitted, driven by its own worker thread of the library, collected in order --
	the host touches a batch twice.
	"""
	from collections import deque
	# four streams per slot (three of the engine's pool and a copy stream): beyond ~24 streams in the process its hardware queues
	# are oversubscribed and time-sliced -- measured in round 5: 3.8-4.2 x 10^5 targets/s with four or five jobs in flight, 2.4-2.9 x 10^5 with six
	in_flight = max(1, min(int(in_flight), FramesEngine.MAX_SLOTS))
	eng = FramesEngine.of(ctx, slots=in_flight)
	cat = eng.catalog(catalog)
	# results are yielded in the order of the batches, but a slot is handed on as soon as ANY job is done: the jobs of a run take
	# 5 - 15 ms each (three to ten groups, one to five rounds), and waiting for the oldest left finished ones holding their slots
	queue, finished, serial, next_out = deque(), {}, 0, 0
	for targets in batches:
		while len(queue) >= in_flight:
			# (at most in_flight results wait for an older batch: beyond that the oldest job is waited for)
			k = 0 if len(finished) >= in_flight else next((k for k, (_, job) in enumerate(queue) if job.done()), 0)
			s, job = queue[k]
			del queue[k]
			finished[s] = job.collect()
			while next_out in finished:
				yield finished.pop(next_out)
				next_out += 1
		queue.append((serial, eng.submit(stack, targets, cat, time, quality, settings=settings, datasource=datasource, budget_share=1.0 / in_flight)))
		serial += 1
	while queue:
		s, job = queue.popleft()
		finished[s] = job.collect()
		while next_out in finished:
			yield finished.pop(next_out)
			next_out += 1


#--------------------------------------------------------------------------------------------------
# PSF photometry of many targets of one CCD region (the batched counterparts of the LinPSF / PSF plugins)
#--------------------------------------------------------------------------------------------------
class PSFFramesResult(object):
	"""
	Columnar results of :func:`linpsf_frames` / :func:`psf_frames`: ``status`` int32 (values of ``STATUS``), ``stamp`` int64
	``(n, 4)``, ``flux`` / ``flux_err`` float64 ``(n, T)``, ``contamination`` float64 (LinPSF), ``pos_centroid`` float64
	``(n, T, 2)`` as (row, column) (PSF), ``errors``: target index -> messages.  ``result[i]`` is the per-target dict.
	"""
	def __init__(self, n, T, method):
		self.n, self.method = n, method
		self.status = np.zeros(n, dtype='int32')
		self.stamp = np.zeros((n, 4), dtype='int64')
		if method == 'linpsf':
			# (filled group by group; the rows no group covers -- invalid stamps -- get their NaN at the end, finish(): two arrays of
			# 21 MB per 2 000 targets are not written twice)
			self.flux, self.flux_err = np.empty((n, T)), np.empty((n, T))
			self._covered = np.zeros(n, dtype=bool)
		else:
			self.flux = np.full((n, T), np.nan)
			self.flux_err = np.full((n, T), np.nan)
			self._covered = None
		self.contamination = np.full(n, np.nan)
		self.pos_centroid = np.full((n, T, 2), np.nan) if method == 'psf' else None
		self.errors = {}

	def finish(self):
		"""NaN for the rows no group has written (see ``__init__``)."""
		if self._covered is not None:
			rest = ~self._covered
			if rest.any():
				self.flux[rest] = np.nan
				self.flux_err[rest] = np.nan
			self._covered = None
		return self

	def __len__(self):
		return self.n

	def __getitem__(self, i):
		i = int(i)
		r = {'status': int(self.status[i]), 'stamp': tuple(int(v) for v in self.stamp[i]), 'errors': list(self.errors.get(i, [])),
			'flux': self.flux[i], 'flux_err': self.flux_err[i]}
		if self.method == 'linpsf':
			r['contamination'] = float(self.contamination[i])
		else:
			r['pos_centroid'] = self.pos_centroid[i]
		return r


def _psf_frame_groups(stack, targets):
	"""Default stamps of the targets (BasePhotometry.py:541-564, no resizing: neither PSF plugin resizes) grouped by size."""
	from . import stamps as st
	first, valid = st.default_stamps(targets['row'], targets['column'], targets['tmag'], stack.limits)
	cur = np.asarray(first, dtype='int64')
	active = np.flatnonzero(valid)
	keys = (cur[active, 1] - cur[active, 0]) * 100000 + (cur[active, 3] - cur[active, 2])
	groups = [(int(key // 100000), int(key % 100000), active[keys == key]) for key in np.unique(keys)]
	return cur, valid, groups


def _jitter32(jitter, T):
	"""Per-cadence (column, row) shifts as the plugins apply them (``catalog_attime``: float32 additions)."""
	if jitter is None:
		return np.zeros(T, dtype='float32'), np.zeros(T, dtype='float32')
	j = np.asarray(jitter, dtype='float64')
	return j[:, 0].astype('float32'), j[:, 1].astype('float32')


def linpsf_frames(ctx, stack, targets, catalog, time, quality, prf_model, jitter=None, cutoff_radius=5, movement=None, timecorr=None, flux_errors=False):
	"""
	``LinPSFPhotometry.do_photometry`` (linpsf_photometry.py:79-219) for every target of a CCD region held in a
	:class:`FrameStack`: default stamps grouped by size and cut on the device, the stars fitted beside each target selected as
	the plugin does (:93-104), their positions at every cadence = catalogue position + ``jitter[k]`` (``(T, 2)`` column / row
	shifts: what ``catalog_attime`` returns for a translation), one ``tp_linpsf_prf`` + ``tp_linpsf_fit`` per group.
	Status and messages follow the plugin: ERROR "All target flux values are NaN.", WARNING "High contamination" above 0.1.
	``movement``: a :class:`~photometry_amd.motion.MovementKernel` with a loaded series instead of ``jitter``.  For a translation the
	shifts are ``movement.jitter(time - timecorr, 0.0, 0.0)`` (frames whose ECC failed come out interpolated, as ``load_series`` does).
	Under a ``'euclidian'`` or ``'affine'`` kernel every star moves by its own shift (``'unchanged'``: by none): ``catalog_attime``'s
	``interpolate`` over each stamp's catalogue, formed on the device in its float32 arithmetic (``tp_motion_star_positions``).
	A ``'wcs'`` kernel does the same through the headers, each stamp's catalogue one batch (``tp_wcs_star_positions``).
	``flux_errors``: also cut the ``images_err`` stack and fill ``flux_err`` with the pixel errors propagated through the fit
	(``tp_linpsf_flux_err``, with the positions the fit used); by default it is NaN as the reference leaves it (linpsf_photometry.py:169).
	Returns a :class:`PSFFramesResult`.
	"""
	from . import psf as hpsf
	n, T = len(targets['starid']), stack.n_cad
	wcs_pairs = series_times = None
	if movement is not None:
		if jitter is not None:
			raise ValueError("give either jitter or movement, not both")
		if movement.warpmode not in ('unchanged', 'translation', 'euclidian', 'affine', 'wcs'):
			raise ValueError(f"linpsf_frames: unknown warpmode '{movement.warpmode}'")
		t = np.asarray(time, dtype='float64')
		t = t if timecorr is None else t - np.asarray(timecorr, dtype='float64')
		if movement.warpmode == 'wcs':
			# per-star shifts: the frame pair of every cadence (interpolate's rule), the positions formed on the device per stamp
			movement._wcs_needs_series()
			wcs_pairs = movement._wcs_frame_pairs(t)
		elif movement.warpmode != 'translation':
			# per-star shifts from the loaded series (on the device once per load_series), the positions formed there per stamp group
			movement.device_series(ctx)
			series_times = t
		else:
			# float positions: jitter() builds its position array from them, and integer ones would truncate the shifts
			jitter = movement.jitter(t, 0.0, 0.0)
	catalog = {k: np.asarray(v) for k, v in catalog.items()}
	out = PSFFramesResult(n, T, 'linpsf')
	cur, valid, groups = _psf_frame_groups(stack, targets)
	out.stamp[:] = cur
	for i in np.flatnonzero(~valid):
		out.status[i] = 2
		out.errors[int(i)] = ['ValueError: Invalid stamp selected']
		out.stamp[i] = (-1, -2, -1, -2)
	cat_index = _CatalogIndex(catalog)
	jc, jr = _jitter32(jitter, T)
	d_jc, d_jr = ctx.array(jc), ctx.array(jr)
	base_coef, tx, ty = ctx.array(prf_model.base_coef), ctx.array(prf_model.tx), ctx.array(prf_model.ty)
	for H, W, idx in groups:
		cat_offsets, cat = _catalogs_of_stamps(cat_index, cur[idx])
		sel, star_offsets, target_index = hpsf.select_stars(cat, cat_offsets, np.asarray(targets['starid'], dtype='int64')[idx])
		# positions = catalogue position + the cadence's shift, summed in float32 like the plugin's catalogue: formed on the device
		# (on the host the two arrays -- 75 MB for 2 000 targets -- were most of this entry's time)
		if series_times is not None:
			# catalog_attime with a euclidian / affine kernel: interpolate() over the float32 catalogue positions, the float32 changes
			# added to the float32 stamp columns (csrc/motion.hip, tp_motion_star_positions)
			rows = np.arange(len(cat['row']))[sel]
			out_index = np.full(len(cat['row']), -1, dtype='int64')
			out_index[rows] = np.arange(len(rows))
			pos_col, pos_row, _ = movement.star_positions(series_times, np.column_stack((cat['column'], cat['row'])), cat['column_stamp'],
				cat['row_stamp'], out_index, len(rows), single=True, ctx=ctx)
		elif wcs_pairs is None:
			pos_row = engine.star_positions(ctx, ctx.array(np.ascontiguousarray(cat['row_stamp'][sel], dtype='float32')), d_jr)
			pos_col = engine.star_positions(ctx, ctx.array(np.ascontiguousarray(cat['column_stamp'][sel], dtype='float32')), d_jc)
		else:
			# catalog_attime with a 'wcs' kernel: every stamp's catalogue is one batch of interpolate(), the jitter added to the
			# float32 stamp columns (csrc/wcs.hip, tp_wcs_star_positions)
			rows = np.arange(len(cat['row']))[sel]
			out_index = np.full(len(cat['row']), -1, dtype='int64')
			out_index[rows] = np.arange(len(rows))
			pos_col, pos_row, _ = wcs.star_positions(ctx, movement._d_series, len(movement.series_kernels), movement.wcs_ref, cat_offsets,
				np.column_stack((cat['column'], cat['row'])), cat['column_stamp'], cat['row_stamp'], out_index, len(rows), *wcs_pairs)
		cube = engine.cut_stamps(ctx, stack.dev['images'], ctx.array(cur[idx].astype('int32')), H, W, stack.row0, stack.col0)
		err_cube = None
		try:
			coef = engine.linpsf_prf(ctx, base_coef, ctx.array(prf_model.weights(cur[idx])))
			d_offsets, d_index, max_stars = ctx.array(star_offsets), ctx.array(target_index), max(int(np.diff(star_offsets).max()), 1)
			fit = engine.linpsf_fit(ctx, cube, coef, tx, ty, d_offsets, d_index, pos_row, pos_col, max_stars, cutoff_radius=cutoff_radius)
			if flux_errors:
				err_cube = engine.cut_stamps(ctx, stack.dev['images_err'], ctx.array(cur[idx].astype('int32')), H, W, stack.row0, stack.col0)
				engine.linpsf_flux_err(ctx, cube, err_cube, coef, tx, ty, d_offsets, d_index, pos_row, pos_col, max_stars, cutoff_radius=cutoff_radius,
					out=fit.flux_err)
			res = fit.to_host(('contamination', 'status'))
			if len(idx) == n and np.array_equal(idx, np.arange(n)) and fit.flux.shape == out.flux.shape:
				# one group holds every target in order (the usual case: default stamps of one size): straight into the result arrays
				fit.flux.to_host(out=out.flux)
				fit.flux_err.to_host(out=out.flux_err)
			else:
				out.flux[idx] = fit.flux.to_host()[:, :T]
				out.flux_err[idx] = fit.flux_err.to_host()[:, :T]
			out._covered[idx] = True
		finally:
			ctx.sync()
			cube.free()
			if err_cube is not None:
				err_cube.free()
		out.contamination[idx] = res['contamination']
		# linpsf_photometry.py:198-200, 214-219: ERROR when every flux is NaN, WARNING above 10 % contamination (NaN compares false)
		failed = res['status'] == 2
		with np.errstate(invalid='ignore'):
			high = ~failed & (res['contamination'] > 0.1)
		out.status[idx] = np.where(failed, 2, np.where(high, 3, 1))
		for i in idx[failed]:
			out.errors[int(i)] = ['All target flux values are NaN.']
		for i in idx[high]:
			out.errors[int(i)] = ['High contamination']
	return out.finish()


def psf_frames(ctx, stack, targets, catalog, time, quality, prf_model, readnoise=10.0, gain=100.0, n_readout=720, cutoff_radius=5, flux_errors=False):
	"""
	``PSFPhotometry.do_photometry`` (psf_photometry.py:111-196) for every target of a CCD region held in a :class:`FrameStack`:
	default stamps grouped by size, images and backgrounds cut on the device, per target the up to five stars the plugin fits
	(:117-130) with their catalogue positions and fluxes as the first guess, the 3 x 3 minimum aperture of the finite sum-image
	pixels (:29-41), one ``tp_psf_fit`` per group (the cadences of a target are a warm-start chain, the targets run side by side).
	``flux_errors``: also cut the ``images_err`` stack per stamp group and fill ``flux_err`` with the pixel errors propagated through
	the fit at its own end points (``tp_psf_flux_err``); by default it is NaN as the reference leaves it (:175).
	Returns a :class:`PSFFramesResult` (status OK, as the plugin: NaN fluxes are only logged there, :190-194).
	"""
	from .plugins import psf_star_selection, mag2flux
	n, T = len(targets['starid']), stack.n_cad
	catalog = {k: np.asarray(v) for k, v in catalog.items()}
	out = PSFFramesResult(n, T, 'psf')
	cur, valid, groups = _psf_frame_groups(stack, targets)
	out.stamp[:] = cur
	for i in np.flatnonzero(~valid):
		out.status[i] = 2
		out.errors[int(i)] = ['ValueError: Invalid stamp selected']
		out.stamp[i] = (-1, -2, -1, -2)
	cat_index = _CatalogIndex(catalog)
	base_coef, tx, ty = ctx.array(prf_model.base_coef), ctx.array(prf_model.tx), ctx.array(prf_model.ty)
	full_sumimage = stack.sumimage_for(quality)
	trow, tcol, ttmag = (np.asarray(targets[k], dtype='float64') for k in ('row', 'column', 'tmag'))
	for H, W, idx in groups:
		cat_offsets, cat = _catalogs_of_stamps(cat_index, cur[idx])
		stamps_dev = ctx.array(cur[idx].astype('int32'))
		images = engine.cut_stamps(ctx, stack.dev['images'], stamps_dev, H, W, stack.row0, stack.col0)
		backgrounds = engine.cut_stamps(ctx, stack.dev['backgrounds'], stamps_dev, H, W, stack.row0, stack.col0)
		err_cube = None
		try:
			# bit 1 of the aperture image (BasePhotometry.py:1033-1074) from the sum image -- for an FFI target a crop of the region's (:1001-1006)
			finite = np.isfinite(engine.crop_sumimage(ctx, full_sumimage, stamps_dev, H, W, stack.row0, stack.col0).to_host()).reshape(len(idx), H, W)
			offsets = [0]
			params0 = []
			mini = np.zeros((len(idx), H, W), dtype='uint8')
			for j, i in enumerate(idx):
				lo, hi = int(cat_offsets[j]), int(cat_offsets[j + 1])
				r1, c1 = cur[i, 0], cur[i, 2]
				sel = psf_star_selection(cat['row_stamp'][lo:hi], cat['column_stamp'][lo:hi], cat['tmag'][lo:hi], trow[i] - r1, tcol[i] - c1, ttmag[i])
				params0.append(np.column_stack((np.asarray(cat['row_stamp'][lo:hi][sel], dtype='float64'), np.asarray(cat['column_stamp'][lo:hi][sel], dtype='float64'),
					mag2flux(np.asarray(cat['tmag'][lo:hi][sel], dtype='float64')))))
				offsets.append(offsets[-1] + len(sel))
				cols, rows = np.meshgrid(np.arange(c1 + 1, cur[i, 3] + 1, dtype='int32'), np.arange(r1 + 1, cur[i, 1] + 1, dtype='int32'))
				mini[j] = (np.abs(cols - tcol[i] - 1) <= 1) & (np.abs(rows - trow[i] - 1) <= 1) & finite[j]
			coef = engine.linpsf_prf(ctx, base_coef, ctx.array(prf_model.weights(cur[idx])))
			d_offsets, d_mini = ctx.array(np.asarray(offsets, dtype='int64')), ctx.array(mini)
			res = engine.psf_fit(ctx, images, backgrounds, coef, tx, ty, d_offsets, ctx.array(np.concatenate(params0, axis=0)),
				d_mini, variance_floor=n_readout * readnoise**2 / gain**2, cutoff_radius=cutoff_radius)
			if flux_errors:
				err_cube = engine.cut_stamps(ctx, stack.dev['images_err'], stamps_dev, H, W, stack.row0, stack.col0)
				engine.psf_flux_err(ctx, images, backgrounds, err_cube, coef, tx, ty, d_offsets, res['params'], d_mini,
					variance_floor=n_readout * readnoise**2 / gain**2, cutoff_radius=cutoff_radius, out=res['flux_err'])
			flux, flux_err = res['flux'].to_host(), res['flux_err'].to_host()
			crow, ccol = res['centroid_row'].to_host(), res['centroid_col'].to_host()
		finally:
			ctx.sync()
			images.free()
			backgrounds.free()
			if err_cube is not None:
				err_cube.free()
		out.flux[idx] = flux[:, :T]
		out.flux_err[idx] = flux_err[:, :T]
		out.pos_centroid[idx, :, 0] = crow[:, :T]
		out.pos_centroid[idx, :, 1] = ccol[:, :T]
		out.status[idx] = 1
	return out


#--------------------------------------------------------------------------------------------------
# Halo photometry of many targets of one CCD region (the batched counterpart of the Halo plugin)
#--------------------------------------------------------------------------------------------------
class HaloFramesResult(object):
	"""
	Columnar results of :func:`halo_frames`: ``status`` int32 (values of ``STATUS``), ``stamp`` int64 ``(n, 4)``, ``flux`` /
	``flux_err`` / ``corr_flux`` float64 ``(n, T)``, ``pos_centroid`` float64 ``(n, T, 2)`` as (column, row), per target the lists
	``pixel_mask`` (= ``final_phot_mask``), ``weightmap`` (the dict ``halo.photometry`` returns), ``w``, ``skip_targets`` and
	``diagnostics`` (OK targets), ``f`` / ``iterations`` / ``tv_status`` ``(n, n_seg)``, ``split_times``, ``segments``, ``headers``
	(the ``HALO_*`` cards), ``errors``: target index -> messages.  ``result[i]`` is the per-target dict.
	"""
	def __init__(self, n, T):
		self.n = int(n)
		self.status = np.zeros(n, dtype='int32')
		self.stamp = np.full((n, 4), -1, dtype='int64')
		self.flux, self.flux_err, self.corr_flux = np.zeros((n, T)), np.zeros((n, T)), np.full((n, T), np.nan)
		self.pos_centroid = np.zeros((n, T, 2))
		self.pixel_mask, self.weightmap, self.w = [None] * n, [None] * n, [None] * n
		self.skip_targets, self.diagnostics = [[] for _ in range(n)], [None] * n
		self.f = self.iterations = self.tv_status = None
		self.split_times = self.segments = None
		self.headers = {}
		self.errors = {}

	def __len__(self):
		return self.n

	def __getitem__(self, i):
		i = int(i)
		if i < 0:
			i += self.n
		if not 0 <= i < self.n:
			raise IndexError(i)
		r = {'status': int(self.status[i]), 'stamp': tuple(int(v) for v in self.stamp[i]), 'errors': list(self.errors.get(i, [])),
			'flux': self.flux[i], 'flux_err': self.flux_err[i], 'corr_flux': self.corr_flux[i], 'pos_centroid': self.pos_centroid[i],
			'pixel_mask': self.pixel_mask[i], 'weightmap': self.weightmap[i], 'w': self.w[i], 'skip_targets': list(self.skip_targets[i]),
			'diagnostics': self.diagnostics[i], 'headers': self.headers}
		if self.f is not None:
			r.update(f=self.f[i], iterations=self.iterations[i], tv_status=self.tv_status[i])
		return r

	def __iter__(self):
		return (self[i] for i in range(self.n))


def halo_frames(ctx, stack, targets, catalog, time, quality, sector=None, timecorr=None, cadenceno=None, jitter=None, settings=None,
	budget_bytes=None):
	"""
	``HaloPhotometry.do_photometry`` (halo/halo_photometry.py:99-265) for every target of a CCD region held in a :class:`FrameStack`
	-- ``tessphot('halo', ...)`` for a batch: the Halo stamps and pixel masks as the plugin forms them, the problems of all targets
	built on the device from the stack, ONE ``tp_halo_tvmin`` call, light curves, flux errors and weight maps formed on the device
	(``halo.photometry_frames``).  ``jitter``: ``(T, 2)`` column / row shifts (``pos_corr``) added to the target position for
	``pos_centroid``; no centroid is computed (:162-164).  Status and messages follow the plugin: ERROR "Halo optimization failed"
	for a degenerate segment, ERROR "no usable pixels in the pixel mask".  Raises ``NotImplementedError`` while ``[halo] enabled``
	is off.  Returns a :class:`HaloFramesResult`.
	"""
	from . import halo
	from .plugins import load_settings
	settings = load_settings() if settings is None else settings
	if not halo.enabled(settings):
		raise NotImplementedError("HaloPhotometry is off: set '[halo] enabled = true' in the settings file named by "
			"TESSPHOT_SETTINGS to run this engine's TV-min implementation")
	n, T = len(targets['starid']), stack.n_cad
	time = np.asarray(time, dtype='float64')
	res = halo.photometry_frames(ctx, stack, targets, time, quality, sector=sector, timecorr=timecorr, cadenceno=cadenceno, budget_bytes=budget_bytes)
	out = HaloFramesResult(n, T)
	out.stamp[:] = res['stamp']
	out.split_times, out.segments = res['split_times'], res['segments']
	out.f, out.iterations, out.tv_status = res['f'], res['iterations'], res['status']
	out.corr_flux, out.flux_err = res['corr_flux'], res['flux_err']
	out.pixel_mask, out.w = res['pixel_mask'], res['w']
	out.headers = {'HALO_VER': (halo.VERSION, 'Version of halo photometry'), 'HALO_OBJ': (halo.SETTINGS['objective'], 'Halophot objective function'),
		'HALO_THR': (halo.SETTINGS['thresh'], 'Halophot saturated pixel threshold'), 'HALO_MXI': (halo.SETTINGS['maxiter'], 'Halophot maximum optimisation iterations'),
		'HALO_SCL': (halo.SETTINGS['sigclip'], 'Halophot sigma clipping enabled'), 'HALO_MFL': (halo.SETTINGS['minflux'], 'Halophot minimum flux')}
	good = np.isfinite(time)
	jit = np.zeros((T, 2)) if jitter is None else np.asarray(jitter, dtype='float64')
	rows, cols = np.asarray(targets['row'], dtype='float64'), np.asarray(targets['column'], dtype='float64')
	n_seg = res['f'].shape[1]
	catalog = {k: np.asarray(v) for k, v in catalog.items()}
	for i in range(n):
		if not res['valid'][i]:
			out.status[i] = STATUS.ERROR.value
			out.errors[i] = ['ValueError: Invalid stamp selected']
			out.stamp[i] = (-1, -2, -1, -2)
		elif n_seg == 0 or not res['usable'][i]:
			out.status[i] = STATUS.ERROR.value
			out.errors[i] = ['ValueError: Halo photometry: no usable pixels in the pixel mask']
		elif np.any(res['status'][i] == halo.DEGENERATE):
			out.status[i] = STATUS.ERROR.value
			out.errors[i] = ['ERROR: Halo optimization failed']
		else:
			out.status[i] = STATUS.OK.value
			out.flux[i, good] = res['flux'][i, good]
			# the target position per cadence; no centroids are calculated (:162-164, :221-222)
			out.pos_centroid[i, :, 0] = cols[i] + jit[:, 0]
			out.pos_centroid[i, :, 1] = rows[i] + jit[:, 1]
			out.weightmap[i] = {'weightmap': res['weightmap'][i], 'initial_cadence': list(res['initial_cadence']),
				'final_cadence': list(res['final_cadence']), 'sat_pixels': [0] * n_seg}
			# other targets in the mask (:257-262)
			st, mask = out.stamp[i], res['pixel_mask'][i]
			cat = _catalog_of_stamp(catalog, st)
			cc, rr = np.meshgrid(np.arange(st[2] + 1, st[3] + 1, 1, dtype='int32'), np.arange(st[0] + 1, st[1] + 1, 1, dtype='int32'))
			out.skip_targets[i] = [int(sid) for sid, r, c in zip(cat['starid'], cat['row'], cat['column'])
				if sid != targets['starid'][i] and np.any(mask & (rr == np.round(r) + 1) & (cc == np.round(c) + 1))]
	# the light-curve diagnostics of the OK targets (BasePhotometry.py:1343-1407), one device call per stamp size
	ok = np.flatnonzero(out.status == STATUS.OK.value)
	if len(ok):
		d_time, d_q = ctx.array(time), ctx.array(np.ascontiguousarray(quality, dtype='int32'))
		keys = (out.stamp[ok, 1] - out.stamp[ok, 0]) * 100000 + (out.stamp[ok, 3] - out.stamp[ok, 2])
		for key in np.unique(keys):
			idx = ok[keys == key]
			H, W = int(key // 100000), int(key % 100000)
			block = np.zeros((5, len(idx), T))
			block[0], block[1] = out.flux[idx], out.flux_err[idx]
			block[3], block[4] = out.pos_centroid[idx, :, 0], out.pos_centroid[idx, :, 1]
			d_st = ctx.array(out.stamp[idx].astype('int32'))
			d_sum = engine.crop_sumimage(ctx, stack.sumimage_for(quality), d_st, H, W, stack.row0, stack.col0)
			d_mask = ctx.array(np.stack([out.pixel_mask[i] for i in idx]).astype('uint8'))
			d_status = ctx.array(np.full(len(idx), STATUS.OK.value, dtype='int32'))
			d_block = ctx.array(block)
			lc = engine.LightCurves(ctx, len(idx), T, block=d_block)
			diag = engine.lightcurve_diagnostics(ctx, lc, d_time, d_q, status=d_status, sumimage=device_view(ctx, d_sum.ptr, (len(idx), H, W), 'float64', base=d_sum),
				mask=d_mask)
			host = diag.to_host()
			for j, i in enumerate(idx):
				out.diagnostics[i] = dict(zip(engine.DIAGNOSTICS_COLUMNS, host[j]))
			for a in (diag, d_block, d_status, d_mask, d_sum, d_st):
				a.free()
		d_time.free()
		d_q.free()
	return out


class HaloResultsOfGroups(object):
	"""The :class:`HaloFramesResult` s of several groups of target pixel files (:func:`halo_tpfs`; the groups differ in stamp shape or
	number of cadences) as one result: row ``r`` is row ``places[r][1]`` of ``parts[places[r][0]]``.  What ``BatchResults.switch_to_halo``
	and the light-curve writer read: ``status``, ``stamp``, ``diagnostics``, ``headers``, ``result[r]``."""
	def __init__(self, parts, places):
		self.parts, self.places = list(parts), [(int(g), int(j)) for g, j in places]
		self.n = len(self.places)
		self.status = np.array([self.parts[g].status[j] for g, j in self.places], dtype='int32')
		self.stamp = np.array([self.parts[g].stamp[j] for g, j in self.places], dtype='int64').reshape(self.n, 4)
		self.diagnostics = [self.parts[g].diagnostics[j] for g, j in self.places]
		self.headers = self.parts[0].headers if self.parts else {}

	def __len__(self):
		return self.n

	def __getitem__(self, r):
		g, j = self.places[int(r)]
		return self.parts[g][j]

	def __iter__(self):
		return (self[r] for r in range(self.n))


def _halo_headers():
	from . import halo
	return {'HALO_VER': (halo.VERSION, 'Version of halo photometry'), 'HALO_OBJ': (halo.SETTINGS['objective'], 'Halophot objective function'),
		'HALO_THR': (halo.SETTINGS['thresh'], 'Halophot saturated pixel threshold'), 'HALO_MXI': (halo.SETTINGS['maxiter'], 'Halophot maximum optimisation iterations'),
		'HALO_SCL': (halo.SETTINGS['sigclip'], 'Halophot sigma clipping enabled'), 'HALO_MFL': (halo.SETTINGS['minflux'], 'Halophot minimum flux')}


def halo_tpfs(ctx, group, idx, catalogs, positions, starid=None, sumimage=None, settings=None, budget_bytes=None):
	"""
	``HaloPhotometry.do_photometry`` for the slots ``idx`` of a ``tpf.TpfGroup`` whose cubes are resident on the device --
	``tessphot('halo', starid, TpfStampSource(...), datasource='tpf')`` for many files of one shape: the problems of all chosen targets
	built on the device from the group's cubes, ONE ``tp_halo_tvmin`` call per chunk, light curves, flux errors and weight maps formed
	there too (``halo.photometry_cubes``).  The stamp is the file's ``max_stamp`` (the plugin resizes for ``'ffi'`` only), the pixel mask
	``halo.pixel_mask`` of the file's aperture image, ``pos_centroid`` the target position plus the file's ``pos_corr``; split times and
	segments are every file's own.  ``catalogs``: per chosen slot the stars of its stamp (``starid, row, column``); ``positions``:
	``(len(idx), 3)`` row, column and Tmag of the main targets; ``starid``: their star numbers (``skip_targets`` lists the others in
	the mask); ``sumimage``: ``(len(idx), H, W)`` the sum images of the chosen slots (the group's aperture pass has them) for the
	light-curve diagnostics, which run with every target's own time row (``tp_lightcurve_diagnostics_times``).  Status and messages are
	the plugin's: ERROR "Halo optimization failed", ERROR "no usable pixels in the pixel mask".  Raises ``NotImplementedError`` while
	``[halo] enabled`` is off.  Returns a :class:`HaloFramesResult` over ``idx`` (``f`` / ``iterations`` / ``tv_status`` /
	``split_times`` / ``segments``: one entry per target).
	"""
	from . import halo
	from .plugins import load_settings, mag2flux
	settings = load_settings() if settings is None else settings
	if not halo.enabled(settings):
		raise NotImplementedError("HaloPhotometry is off: set '[halo] enabled = true' in the settings file named by "
			"TESSPHOT_SETTINGS to run this engine's TV-min implementation")
	idx = [int(s) for s in idx]
	n, m = len(group), len(idx)
	H, W, T = group.shape
	positions = np.asarray(positions, dtype='float64').reshape(m, 3)
	starid = [None] * m if starid is None else [int(s) for s in starid]
	masks = np.zeros((n, H, W), dtype=bool)
	normfactor = np.ones(n)
	grids = []
	for j, s in enumerate(idx):
		st = group.loaded[s].max_stamp
		cols, rows = np.meshgrid(np.arange(st[2] + 1, st[3] + 1, 1, dtype='int32'), np.arange(st[0] + 1, st[1] + 1, 1, dtype='int32'))
		grids.append((cols, rows))
		masks[s] = halo.pixel_mask(group.aperture[s], cols, rows, positions[j, 0], positions[j, 1])
		normfactor[s] = mag2flux(float(positions[j, 2]))                    # (one scalar call per target, as the plugin makes it)
	timecorr = np.stack([np.asarray(ld.timecorr, dtype='float64') for ld in group.loaded])
	cadenceno = np.stack([np.asarray(ld.cadenceno) for ld in group.loaded])
	sector = np.array([-1 if ld.sector is None else int(ld.sector) for ld in group.loaded])
	res = halo.photometry_cubes(ctx, group.cubes, masks, group.time, timecorr, cadenceno, group.quality, sector, normfactor,
		budget_bytes=budget_bytes, targets=idx)
	out = HaloFramesResult(m, T)
	out.headers = _halo_headers()
	out.f, out.iterations, out.tv_status = ([res[k][s] for s in idx] for k in ('f', 'iterations', 'status'))
	out.split_times, out.segments = [res['split_times'][s] for s in idx], [res['segments'][s] for s in idx]
	for j, s in enumerate(idx):
		ld = group.loaded[s]
		out.stamp[j] = ld.max_stamp
		out.corr_flux[j], out.flux_err[j] = res['corr_flux'][s], res['flux_err'][s]
		out.pixel_mask[j], out.w[j] = masks[s], res['w'][s]
		messages = list(res['messages'][s])                                 # (the warnings of the split times: the plugin's log keeps them)
		if not res['usable'][s]:
			out.status[j] = STATUS.ERROR.value
			out.errors[j] = messages + ['ValueError: Halo photometry: no usable pixels in the pixel mask']
		elif np.any(res['status'][s] == halo.DEGENERATE):
			out.status[j] = STATUS.ERROR.value
			out.errors[j] = messages + ['ERROR: Halo optimization failed']
		else:
			out.status[j] = STATUS.OK.value
			if messages:
				out.errors[j] = messages
			good = np.isfinite(group.time[s])
			out.flux[j, good] = res['flux'][s][good]
			# the target position per cadence; no centroids are calculated (:162-164, :221-222)
			jit = np.asarray(ld.pos_corr, dtype='float64')
			out.pos_centroid[j, :, 0] = positions[j, 1] + jit[:, 0]
			out.pos_centroid[j, :, 1] = positions[j, 0] + jit[:, 1]
			k = len(res['status'][s])
			out.weightmap[j] = {'weightmap': res['weightmap'][s], 'initial_cadence': list(res['initial_cadence'][s]),
				'final_cadence': list(res['final_cadence'][s]), 'sat_pixels': [0] * k}
			# other targets in the mask (:257-262)
			cat, (cc, rr) = catalogs[j], grids[j]
			out.skip_targets[j] = [int(sid) for sid, r, c in zip(cat['starid'], cat['row'], cat['column'])
				if sid != starid[j] and np.any(masks[s] & (rr == np.round(r) + 1) & (cc == np.round(c) + 1))]
	# the light-curve diagnostics of the OK targets (BasePhotometry.py:1343-1407), every target on its own time axis: one device call
	ok = np.flatnonzero(out.status == STATUS.OK.value)
	if len(ok):
		slots = [idx[j] for j in ok]
		block = np.zeros((5, len(ok), T))
		block[0], block[1] = out.flux[ok], out.flux_err[ok]
		block[3], block[4] = out.pos_centroid[ok, :, 0], out.pos_centroid[ok, :, 1]
		sums = np.full((len(ok), H, W), np.nan) if sumimage is None else np.ascontiguousarray(np.asarray(sumimage, dtype='float64').reshape(m, H, W)[ok])
		d_time, d_q = ctx.array(np.ascontiguousarray(group.time[slots])), ctx.array(np.ascontiguousarray(group.quality[slots], dtype='int32'))
		d_sum, d_mask = ctx.array(sums), ctx.array(np.stack([out.pixel_mask[j] for j in ok]).astype('uint8'))
		d_status = ctx.array(np.full(len(ok), STATUS.OK.value, dtype='int32'))
		d_block = ctx.array(block)
		lc = engine.LightCurves(ctx, len(ok), T, block=d_block)
		diag = engine.lightcurve_diagnostics(ctx, lc, d_time, d_q, status=d_status, sumimage=d_sum, mask=d_mask)
		host = diag.to_host()
		for r, j in enumerate(ok):
			out.diagnostics[j] = dict(zip(engine.DIAGNOSTICS_COLUMNS, host[r]))
		for a in (diag, d_block, d_status, d_mask, d_sum, d_time, d_q):
			a.free()
	return out


#--------------------------------------------------------------------------------------------------
# LinPSF photometry of many target pixel files of one shape (the batched counterpart of the LinPSF plugin on a ``tpf`` source)
#--------------------------------------------------------------------------------------------------
class LinPSFTpfsResult(PSFFramesResult):
	"""
	Columnar results of :func:`linpsf_tpfs` over the chosen slots of a group: what :class:`PSFFramesResult` holds for ``'linpsf'``, the
	``status`` and ``errors`` final -- with what ``BasePhotometry.photometry`` makes of the light-curve diagnostics --, plus per target
	``diagnostics`` (the dict of ``engine.DIAGNOSTICS_COLUMNS`` for a target the fit left OK or WARNING, else None), ``n_stars`` (stars
	fitted), ``fitted`` (the target went through the fit: its ``flux`` / ``flux_err`` are the fit's) and ``headers`` (the
	``additional_headers`` of the plugin: ``PSF_FERR``, ``PSF_CONT``).  ``flux_errors``: whether the error pass ran.
	"""
	def __init__(self, n, T, flux_errors):
		super().__init__(n, T, 'linpsf')
		self.flux_errors = bool(flux_errors)
		self.diagnostics = [None] * n
		self.headers = [{} for _ in range(n)]
		self.n_stars = np.zeros(n, dtype='int64')
		self.fitted = np.zeros(n, dtype=bool)

	def __getitem__(self, i):
		i = int(i)
		r = super().__getitem__(i)
		r.update(diagnostics=self.diagnostics[i], headers=dict(self.headers[i]), n_stars=int(self.n_stars[i]), fitted=bool(self.fitted[i]))
		return r


def _prf_models_of_slots(group, slots, prf):
	"""The PRF model of every chosen slot -- ``prf`` itself, ``prf[(camera, ccd)]``, or with ``None`` the SPOC model of the file's sector,
	camera and CCD from ``TESSPHOT_PSF_DIR`` as ``BasePhotometry.psf`` finds it -- or the text of the exception the plugin would die of."""
	import os
	from . import psf as hpsf
	from .plugins import _PRF_CACHE
	models = []
	for s in slots:
		ld = group.loaded[s]
		try:
			if prf is None:
				psf_dir = os.environ.get('TESSPHOT_PSF_DIR')
				if not psf_dir:
					raise FileNotFoundError("the stamp source provides no PRF model and no PRF directory is configured (TESSPHOT_PSF_DIR)")
				key = (os.path.abspath(psf_dir), int(ld.sector), int(ld.camera), int(ld.ccd))
				if key not in _PRF_CACHE:
					_PRF_CACHE[key] = hpsf.PRFModel.for_ccd(psf_dir, ld.sector, ld.camera, ld.ccd)
				models.append(_PRF_CACHE[key])
			elif isinstance(prf, hpsf.PRFModel):
				models.append(prf)
			else:
				models.append(prf[(int(ld.camera), int(ld.ccd))])
		except (FileNotFoundError, ValueError, KeyError, TypeError) as e:
			models.append(f"{type(e).__name__}: {e}")
	return models


def _consecutive_slices(slots, cost, budget):
	"""``slots`` (rising) cut into slices of consecutive slot numbers whose summed ``cost`` stays within ``budget`` (a slice holds at least
	one slot): ``[(first position in slots, count), ...]``."""
	out, a = [], 0
	while a < len(slots):
		b, spent = a + 1, cost[a]
		while b < len(slots) and slots[b] == slots[b - 1] + 1 and spent + cost[b] <= budget:
			spent += cost[b]
			b += 1
		out.append((a, b - a))
		a = b
	return out


def linpsf_tpfs(ctx, group, idx, catalogs, positions, starid, prf, cutoff_radius=5, flux_errors=False, budget_bytes=None):
	"""
	``LinPSFPhotometry.do_photometry`` for the slots ``idx`` of a ``tpf.TpfGroup`` whose cubes are resident on the device --
	``tessphot('linpsf', starid, TpfStampSource(loaded, catalog, prf=model), datasource='tpf')`` for many files of one shape.  The stamp
	is the file's ``max_stamp``; the stars fitted beside each target are selected as the plugin selects them (``psf.select_stars`` over
	the concatenated ``catalogs``: per chosen slot the stars of its stamp with ``starid, tmag, row_stamp, column_stamp``); their positions
	at every cadence are catalogue position + the FILE's ``pos_corr`` at the cadence ``tpf.jitter_lookup`` names, summed in float32 and
	formed on the device from the group's ``pos_corr`` uploaded once (``tp_star_positions_targets``, one call per axis and slice; a file
	whose lookup is not the identity has its stars redone with it); ``tp_linpsf_fit`` runs on ``group.cubes['images']`` as it lies, and with
	``flux_errors`` ``tp_linpsf_flux_err`` on ``group.cubes['images_err']`` with the same device arrays.

	``prf``: a ``psf.PRFModel`` for all files, a mapping ``(camera, ccd) -> PRFModel``, or ``None``: the SPOC model of each file's sector,
	camera and CCD from ``TESSPHOT_PSF_DIR``.  Models that share their knots are fitted in one pass, each slot with the coefficients of
	its own model; models with other knots get a pass of their own over their slots.  ``positions`` (``(len(idx), 3)`` row, column, Tmag
	of the main targets, as :func:`halo_tpfs` takes them) and ``starid``: the main targets.

	Slots that are not in ``idx`` are never handed to a kernel: the fit runs over slices of CONSECUTIVE chosen slots, the cube pointer
	moved to the first slot of a slice.  A slice also ends where its position, per-star flux, flux and flux-error arrays (float64, one
	row of ``T`` per fitted star or target) would pass ``budget_bytes`` (default: a quarter of the device memory free at the call); every
	target is fitted on its own, so where a slice ends changes no bit.

	Status and messages are the plugin's: ERROR "All target flux values are NaN.", WARNING "High contamination" above 0.1, else OK; then
	the light-curve diagnostics of the OK / WARNING targets (one ``tp_lightcurve_diagnostics_times`` launch, every target on its own time
	axis) as ``BasePhotometry.photometry`` reads them: all fluxes or all errors NaN, or an invalid time vector, is ERROR with the
	``ValueError``'s text -- with ``flux_errors`` off that is every target, as in the reference, whose ``flux_err`` is NaN.
	Returns a :class:`LinPSFTpfsResult` over ``idx``.
	"""
	idx = [int(s) for s in idx]
	m = len(idx)
	H, W, T = group.shape
	if any(b <= a for a, b in zip(idx, idx[1:])) or (m and not (0 <= idx[0] and idx[-1] < len(group))):
		raise ValueError("linpsf_tpfs: idx must be rising slot numbers of the group")
	starid = np.asarray(starid, dtype='int64').reshape(m)
	out = LinPSFTpfsResult(m, T, flux_errors)
	for j, s in enumerate(idx):
		out.stamp[j] = group.loaded[s].max_stamp
	# what a target cannot be fitted without: its model and itself among its stars (the plugin dies of the exception; so does the target)
	models = _prf_models_of_slots(group, idx, prf)
	fit = []
	for j in range(m):
		if isinstance(models[j], str):
			out.status[j], out.errors[j] = STATUS.ERROR.value, [models[j]]
		elif not np.any(np.asarray(catalogs[j]['starid']) == starid[j]):
			out.status[j], out.errors[j] = STATUS.ERROR.value, ['ValueError: main target missing from its catalog']
		else:
			fit.append(j)
	# one pass per set of models with the same knots
	passes = []
	for j in fit:
		for p in passes:
			ref = models[p[0]]
			if models[j] is ref or (np.array_equal(models[j].tx, ref.tx) and np.array_equal(models[j].ty, ref.ty)):
				p.append(j)
				break
		else:
			passes.append([j])
	if budget_bytes is None:
		budget_bytes = ctx.mem_info()[0] / 4.0
	images, images_err = group.cubes['images'], group.cubes['images_err']
	d_shift = None
	try:
		if fit:
			# the group's POS_CORR, once: [n][T] float64 per axis (column, row)
			jit = np.stack([np.asarray(ld.pos_corr, dtype='float64').reshape(T, 2) for ld in group.loaded])
			d_shift = (ctx.array(np.ascontiguousarray(jit[:, :, 0])), ctx.array(np.ascontiguousarray(jit[:, :, 1])))
		for members in passes:
			_linpsf_tpfs_pass(ctx, group, idx, members, catalogs, starid, models, d_shift, images, images_err if flux_errors else None,
				cutoff_radius, budget_bytes, out)
	finally:
		ctx.sync()
		for a in d_shift or ():
			a.free()
	# linpsf_photometry.py:198-200, :214-219: ERROR when every flux is NaN, WARNING above 10 % contamination (NaN compares false)
	for j in fit:
		if flux_errors:
			out.headers[j]['PSF_FERR'] = (True, 'flux errors propagated from pixel errors')
		if out.status[j] == 2:
			out.status[j], out.errors[j] = STATUS.ERROR.value, ['All target flux values are NaN.']
			continue
		contamination = float(out.contamination[j])
		out.headers[j]['PSF_CONT'] = (contamination, 'PSF contamination')
		if contamination > 0.1:
			out.status[j], out.errors[j] = STATUS.WARNING.value, ['High contamination']
		else:
			out.status[j] = STATUS.OK.value
	out.finish()
	# BasePhotometry.photometry (BasePhotometry.py:1343-1407) for the OK / WARNING targets, every target on its own time axis: one launch
	ok = np.array([j for j in fit if out.status[j] in (STATUS.OK.value, STATUS.WARNING.value)], dtype='int64')
	if len(ok):
		slots = [idx[j] for j in ok]
		block = np.zeros((5, len(ok), T))
		block[0], block[1] = out.flux[ok], out.flux_err[ok]                 # (no centroids: the plugin leaves pos_centroid at zero)
		d_time, d_q = ctx.array(np.ascontiguousarray(group.time[slots])), ctx.array(np.ascontiguousarray(group.quality[slots], dtype='int32'))
		d_status, d_block = ctx.array(np.ascontiguousarray(out.status[ok], dtype='int32')), ctx.array(block)
		lc = engine.LightCurves(ctx, len(ok), T, block=d_block)
		diag = engine.lightcurve_diagnostics(ctx, lc, d_time, d_q, status=d_status)
		host = diag.to_host()
		for a in (diag, d_block, d_status, d_time, d_q):
			a.free()
		for r, j in enumerate(ok):
			d = dict(zip(engine.DIAGNOSTICS_COLUMNS, host[r]))
			out.diagnostics[j] = d
			problems = int(d['flags'])
			text = ('ValueError: Final lightcurve fluxes are all NaNs' if problems & 1 else 'ValueError: Final lightcurve errors are all NaNs' if problems & 2
				else 'ValueError: Invalid time-vector specified' if problems & 4 else None)
			if text is not None:
				out.status[j] = STATUS.ERROR.value
				out.errors.setdefault(int(j), []).append(text)
			elif problems & 8:
				out.errors.setdefault(int(j), []).append('WARNING: Could not detrend lightcurve for variability calculation.')
	return out


def _linpsf_tpfs_pass(ctx, group, idx, members, catalogs, starid, models, d_shift, images, images_err, cutoff_radius, budget_bytes, out):
	"""One pass of :func:`linpsf_tpfs`: the chosen targets ``members`` (positions in ``idx``), whose models share their knots, slice by slice."""
	from . import psf as hpsf, tpf
	H, W, T = group.shape
	ref = models[members[0]]
	slots = [idx[j] for j in members]
	# the stars of every member, as the plugin selects them
	counts = [len(catalogs[j]['starid']) for j in members]
	offs = np.concatenate(([0], np.cumsum(counts))).astype('int64')
	cat = {k: np.concatenate([np.asarray(catalogs[j][k]) for j in members]) for k in ('starid', 'tmag', 'row_stamp', 'column_stamp')}
	sel, star_offsets, target_index = hpsf.select_stars(cat, offs, starid[members])
	n_stars = np.diff(star_offsets)
	out.n_stars[members] = n_stars
	base_row = np.ascontiguousarray(cat['row_stamp'][sel], dtype='float32')
	base_col = np.ascontiguousarray(cat['column_stamp'][sel], dtype='float32')
	star_target = np.repeat(np.asarray(slots, dtype='int32'), n_stars).astype('int32')     # (the slot: the row of the group's pos_corr)
	# per member: positions and per-star fluxes of its stars, its flux and flux error -- float64 rows of T
	cost = [(3 * max(int(k), 1) + 2) * T * 8 for k in n_stars]
	# the spline coefficients of every member's slot, each from its own model: [members][n * ny] float64
	by_model = {}
	for r, j in enumerate(members):
		by_model.setdefault(id(models[j]), []).append(r)
	coef = ctx.empty((len(members), ref.base_coef.shape[1]), 'float64')
	tx, ty = ctx.array(ref.tx), ctx.array(ref.ty)
	keep = [coef, tx, ty]
	try:
		for rows in by_model.values():
			model = models[members[rows[0]]]
			d_base = ctx.array(model.base_coef)
			keep.append(d_base)
			a = 0
			while a < len(rows):                                               # (runs of consecutive members: written in place)
				b = a + 1
				while b < len(rows) and rows[b] == rows[b - 1] + 1:
					b += 1
				d_w = ctx.array(model.weights(out.stamp[[members[r] for r in rows[a:b]]]))
				keep.append(d_w)
				engine.linpsf_prf(ctx, d_base, d_w, out=coef.slice0(rows[a], b - a))
				a = b
		lookups = {r: tpf.jitter_lookup(group.loaded[s].time, group.loaded[s].timecorr) for r, s in enumerate(slots)}
		for a, count in _consecutive_slices(slots, cost, budget_bytes):
			rows = np.arange(a, a + count)
			s0, s1 = int(star_offsets[a]), int(star_offsets[a + count])
			nfit = s1 - s0
			d_row, d_col = ctx.array(base_row[s0:s1]), ctx.array(base_col[s0:s1])
			d_tgt = ctx.array(star_target[s0:s1])
			pos_row, pos_col = ctx.empty((max(nfit, 1), T), 'float64'), ctx.empty((max(nfit, 1), T), 'float64')
			held = [d_row, d_col, d_tgt, pos_row, pos_col]
			engine.star_positions_targets(ctx, d_row, d_tgt, d_shift[1], T, out=pos_row)
			engine.star_positions_targets(ctx, d_col, d_tgt, d_shift[0], T, out=pos_col)
			for r in rows:
				if lookups[int(r)] is None or n_stars[r] == 0:
					continue
				# a file whose tref repeats or is not finite: its stars again, through its lookup
				b0, k = int(star_offsets[r]) - s0, int(n_stars[r])
				d_look = ctx.array(lookups[int(r)].reshape(1, T))
				d_zero = ctx.array(np.zeros(k, dtype='int32'))
				held += [d_look, d_zero]
				s = slots[int(r)]
				engine.star_positions_targets(ctx, d_row.slice0(b0, k), d_zero, d_shift[1].slice0(s, 1), T, lookup=d_look, out=pos_row.slice0(b0, k))
				engine.star_positions_targets(ctx, d_col.slice0(b0, k), d_zero, d_shift[0].slice0(s, 1), T, lookup=d_look, out=pos_col.slice0(b0, k))
			d_offsets = ctx.array((star_offsets[a:a + count + 1] - s0).astype('int64'))
			d_index = ctx.array(np.ascontiguousarray(target_index[a:a + count], dtype='int32'))
			held += [d_offsets, d_index]
			max_stars = max(int(n_stars[a:a + count].max()), 1)
			cube = images.slice0(slots[a], count)
			res = engine.linpsf_fit(ctx, cube, coef.slice0(a, count), tx, ty, d_offsets, d_index, pos_row, pos_col, max_stars, cutoff_radius=cutoff_radius)
			held += [res.flux, res.flux_err, res.fluxes_all, res.contamination, res.status, res.fluxes_mean]
			if images_err is not None:
				engine.linpsf_flux_err(ctx, cube, images_err.slice0(slots[a], count), coef.slice0(a, count), tx, ty, d_offsets, d_index, pos_row, pos_col,
					max_stars, cutoff_radius=cutoff_radius, out=res.flux_err)
			host = res.to_host(('flux', 'flux_err', 'contamination', 'status'))
			where = [members[int(r)] for r in rows]
			out.flux[where] = host['flux'][:, :T]
			out.flux_err[where] = host['flux_err'][:, :T]
			out.contamination[where] = host['contamination']
			out.status[where] = host['status']
			out._covered[where] = True
			out.fitted[where] = True
			for x in held:
				x.free()
	finally:
		ctx.sync()
		for x in keep:
			x.free()
