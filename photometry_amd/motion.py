# -*- coding: utf-8 -*-
"""
Image movement kernels (photometry/image_motion.py) on the device.

The prepare stage of the reference measures where the stars are at every cadence: ``ImageMovementKernel.calc_kernel``
(image_motion.py:182-256) registers every FFI of a CCD against a reference frame with OpenCV's ECC maximisation
(``cv2.findTransformECC``) on a Scharr-gradient image (``_prepare_flux``, :74-110) and stores the warps as the
``movement_kernel`` dataset (prepare.py:678-697).  Everything downstream reads them through ``load_series`` /
``interpolate`` / ``jitter`` (:259-421): ``catalog_attime`` (BasePhotometry.py:1224-1258) and the ``pos_corr`` column (:473).

:class:`MovementKernel` has the public surface of ``ImageMovementKernel``; its ``calc_kernel`` and the batched
:func:`movement_kernels_frames` run on the device (``tp_motion_prepare`` / ``tp_motion_ecc``, csrc/motion.hip).  The
restatement the device is held to is ``tests/motion_common.py``; DESIGN.md section 9 lists the deliberate differences from
OpenCV.

A loaded series is applied to many positions on the device too: ``jitter_many`` (``tp_motion_interpolate`` /
``tp_motion_star_positions``: scipy's interp1d bit for bit, one 2 x 3 matrix per cadence, a streaming pass over the positions), which
``linpsf_frames`` uses for euclidian and affine kernels and ``tessphot_frames(movement=)`` for ``pos_corr``.  ``interpolate``,
``jitter`` and ``apply_kernel`` stay the reference's host arithmetic.

The ``'wcs'`` warpmode -- the reference's default whenever the FFIs carry per-frame WCS headers (BasePhotometry.py:1185-1221) --
takes its kernels from TAN-SIP WCS headers through :mod:`photometry_amd.wcs` (csrc/wcs.hip) instead of astropy.wcs: with a
``wcs_ref`` (header string, card dict or :class:`~photometry_amd.wcs.TanSipWCS`), ``apply_kernel``, ``load_series``,
``interpolate`` and ``jitter`` behave as image_motion.py:131-138, :278-313, :357-421 (``jitter`` evaluates every frame in one
launch).  Without a ``wcs_ref`` the mode still raises ``NotImplementedError`` ("needs astropy.wcs") wherever it would be used.
"""

import logging
import warnings
import numpy as np
from scipy.interpolate import interp1d

logger = logging.getLogger(__name__)

#: per-frame states written by tp_motion_ecc
STATUS_CONVERGED, STATUS_CAP_REACHED, STATUS_FAILED_NAN, STATUS_FAILED_LAMBDA = 1, 2, 3, 4

#: warpmode -> the TP_MOTION_* code of tp_motion_interpolate / tp_motion_star_positions ('wcs' has its own entries, csrc/wcs.hip)
WARPMODE_CODE = {'unchanged': 0, 'translation': 1, 'euclidian': 2, 'affine': 3}

_WCS_MESSAGE = "warpmode 'wcs' needs astropy.wcs, which this build does not provide"


def _no_wcs():
	raise NotImplementedError(_WCS_MESSAGE)


def _device_stack(ctx, images):
	"""A float32 DeviceArray (T, R, C) of ``images`` (a DeviceArray is used as it is)."""
	if hasattr(images, 'ptr'):
		if np.dtype(images.dtype) != np.dtype('float32') or len(images.shape) != 3:
			raise ValueError("images: float32 stack (T, R, C) expected")
		return images
	a = np.asarray(images, dtype='float32')
	if a.ndim == 2:
		a = a[None]
	if a.ndim != 3:
		raise ValueError("images: float32 stack (T, R, C) expected")
	return ctx.array(np.ascontiguousarray(a))


def prepare_frames(ctx, images):
	"""``_prepare_flux`` of every frame of ``images`` (T, R, C) on the device: a float32 DeviceArray (T, R, C)."""
	d = _device_stack(ctx, images)
	T, R, C = d.shape
	out = ctx.empty((T, R, C), 'float32')
	ctx._check(ctx.lib.tp_motion_prepare(ctx.handle, d.ptr, T, R, C, R * C, out.ptr))
	return out


def _warp_to_kernels(warp, warpmode):
	"""calc_kernel's return values (image_motion.py:241-256) from the (T, 2, 3) warps."""
	if warpmode == 'affine':
		return warp.reshape(len(warp), 6).copy()
	k = np.empty((len(warp), 3 if warpmode == 'euclidian' else 2))
	k[:, 0] = warp[:, 0, 2]
	k[:, 1] = warp[:, 1, 2]
	if warpmode == 'euclidian':
		k[:, 2] = np.arctan2(warp[:, 1, 0], warp[:, 0, 0])
	return k


def ecc_prepared(ctx, template, prepared, warpmode, number_of_iterations=10000, termination_eps=1e-6, chunk_bytes=0):
	"""
	``tp_motion_ecc`` of the prepared frames ``prepared`` (float32 DeviceArray (T, R, C)) against the prepared reference
	``template`` (float32 DeviceArray (R, C) or a view of one frame).  Returns a dict of host arrays: ``kernels`` (T, n_params)
	float64 (NaN where the frame failed), ``warp`` (T, 2, 3), ``rho``, ``iterations``, ``status``.
	"""
	n_params = MovementKernel.N_PARAMS[warpmode]
	T, R, C = prepared.shape
	# tp_motion_ecc reads the template as one frame of the stack's geometry: anything else would be read out of its bounds
	tshape = tuple(template.shape)
	if tshape not in ((R, C), (1, R, C)):
		raise ValueError(f"template of shape {tshape} does not match the frames ({R}, {C})")
	d_warp = ctx.empty((T, 6), 'float64')
	d_rho = ctx.empty((T,), 'float64')
	d_iters = ctx.empty((T,), 'int32')
	d_status = ctx.empty((T,), 'int32')
	ctx._check(ctx.lib.tp_motion_ecc(ctx.handle, template.ptr, prepared.ptr, T, R, C, R * C, n_params, int(number_of_iterations),
		float(termination_eps), int(chunk_bytes), d_warp.ptr, d_rho.ptr, d_iters.ptr, d_status.ptr))
	warp = d_warp.to_host().reshape(T, 2, 3)
	status = d_status.to_host()
	kernels = _warp_to_kernels(warp, warpmode)
	failed = status >= STATUS_FAILED_NAN
	kernels[failed] = np.nan
	for k in np.flatnonzero(failed):
		# image_motion.py:237-239: every exception of findTransformECC gives a NaN kernel
		logger.error("Could not find transform: frame %d: %s", k, "NaN encountered" if status[k] == STATUS_FAILED_NAN else
			"the correlation is going to be minimized; images may be uncorrelated or non-overlapped")
	return {'kernels': kernels, 'warp': warp, 'rho': d_rho.to_host(), 'iterations': d_iters.to_host(), 'status': status}


def movement_kernels_frames(ctx, images, ref_frame, warpmode='translation', number_of_iterations=10000, termination_eps=1e-6, chunk_bytes=0):
	"""
	``ImageMovementKernel(image_ref=images[ref_frame], warpmode=warpmode).calc_kernel`` of every frame of ``images``
	(float32 ``(T, R, C)``, host array or DeviceArray) -- the loop of prepare.py:678-697 in one call.

	Returns a dict of host arrays: ``kernels`` ``(T, n_params)`` float64, NaN where a frame failed (logged as the reference does),
	``rho`` (the last correlation measured), ``iterations`` and ``status`` (1 converged, 2 iteration cap, 3 / 4 failed) per frame,
	and ``warp`` ``(T, 2, 3)``.
	"""
	if warpmode not in MovementKernel.N_PARAMS:
		raise ValueError("Invalid warpmode")
	if warpmode == 'wcs':
		_no_wcs()
	d = _device_stack(ctx, images)
	T = d.shape[0]
	if warpmode == 'unchanged':
		return {'kernels': np.empty((T, 0)), 'warp': np.tile(np.eye(2, 3), (T, 1, 1)), 'rho': np.full(T, np.nan),
			'iterations': np.zeros(T, dtype='int32'), 'status': np.full(T, STATUS_CONVERGED, dtype='int32')}
	ref_frame = int(ref_frame)
	if not 0 <= ref_frame < T:
		raise ValueError(f"ref_frame {ref_frame} outside the stack of {T} frames")
	prepared = prepare_frames(ctx, d)
	try:
		return ecc_prepared(ctx, prepared.slice0(ref_frame, 1), prepared, warpmode, number_of_iterations, termination_eps, chunk_bytes)
	finally:
		ctx.sync()
		prepared.free()


class MovementKernel(object):
	"""
	``ImageMovementKernel`` (image_motion.py:29-421) with ``calc_kernel`` on the device.

	Parameters:
		warpmode (str): ``'wcs'``, ``'unchanged'``, ``'translation'``, ``'euclidian'`` or ``'affine'``.
		image_ref (2D ndarray): the reference image (prepared on the device when a kernel is first computed).
		wcs_ref: the reference WCS of ``'wcs'`` (header string, card dict or :class:`~photometry_amd.wcs.TanSipWCS`); given with
			any other warpmode it raises ``NotImplementedError``.
		ctx: the device :class:`photometry_amd.device.Context` ``calc_kernel`` runs on (default: a context on GPU 0, opened on
			first use).
	"""

	N_PARAMS = {
		'unchanged': 0,
		'translation': 2,
		'euclidian': 3,
		'affine': 6,
		'wcs': 1
	}

	def __init__(self, warpmode='euclidian', image_ref=None, wcs_ref=None, ctx=None):
		if warpmode not in MovementKernel.N_PARAMS:
			raise ValueError("Invalid warpmode")
		self.warpmode = warpmode
		self.n_params = MovementKernel.N_PARAMS[warpmode]
		self.image_ref = None if image_ref is None else np.array(image_ref, dtype='float32')
		if wcs_ref is not None and warpmode != 'wcs':
			_no_wcs()
		self.wcs_ref = None
		if wcs_ref is not None:
			from . import wcs as wcsmod
			self.wcs_ref = wcsmod.as_wcs(wcs_ref, ctx=ctx)
		self.ctx = ctx
		self._template = None
		self._interpolator = None
		self._series_good = None
		self._d_loaded = None

	def __call__(self, *args, **kwargs):
		return self.apply_kernel(*args, **kwargs)

	def _context(self):
		if self.ctx is None:
			from .device import Context
			self.ctx = Context(0)
		return self.ctx

	def apply_kernel(self, xy, kernel):
		"""The change of the positions ``xy`` (rows of column, row) under ``kernel`` (image_motion.py:113-179)."""
		xy = np.atleast_2d(xy)
		delta_pos = np.empty_like(xy)
		if self.warpmode == 'wcs':
			return self._wcs_jitters([kernel], xy)[0]
		elif self.warpmode == 'unchanged':
			delta_pos.fill(0)
		elif self.warpmode == 'translation':
			delta_pos[:, 0] = kernel[0]
			delta_pos[:, 1] = kernel[1]
		else:
			if self.warpmode == 'euclidian':
				c, s = np.cos(kernel[2]), np.sin(kernel[2])
				M = np.array([[c, -s, kernel[0]], [s, c, kernel[1]]])
			else:
				M = np.reshape(kernel, (2, 3))
			# one 3-vector product per position, evaluated like the reference's np.dot(matrix, [x, y, 1])
			for i, (x, y) in enumerate(xy):
				delta_pos[i, :] = np.dot(M, [x, y, 1])
			delta_pos -= xy
		return delta_pos

	def calc_kernel(self, image, number_of_iterations=10000, termination_eps=1e-6):
		"""The movement kernel of ``image`` against the reference image (image_motion.py:182-256), computed on the device."""
		if self.warpmode == 'unchanged':
			return []
		if self.image_ref is None:
			raise RuntimeError("Reference image not defined")
		if self.warpmode == 'wcs':
			_no_wcs()
		if np.shape(image) != self.image_ref.shape:
			# findTransformECC refuses images of another size than the template: the reference logs it and returns NaN
			# (image_motion.py:237-239); nothing goes to the device
			logger.error("Could not find transform: image of shape %s against a reference image of shape %s", np.shape(image),
				self.image_ref.shape)
			return np.full(self.n_params, np.nan)
		ctx = self._context()
		if self._template is None:
			self._template = prepare_frames(ctx, self.image_ref)
		prepared = prepare_frames(ctx, image)
		try:
			res = ecc_prepared(ctx, self._template, prepared, self.warpmode, number_of_iterations, termination_eps)
		finally:
			ctx.sync()
			prepared.free()
		k = res['kernels'][0]
		return k if self.warpmode == 'affine' or not np.all(np.isfinite(k)) else list(k)

	def load_series(self, times, kernels):
		"""Time series of kernels and its interpolator (image_motion.py:259-335); non-finite kernels are left out."""
		if self.warpmode == 'wcs':
			return self._wcs_load_series(times, kernels)
		self.series_times = np.asarray(times)
		self.series_kernels = np.atleast_2d(kernels)
		expected = (len(self.series_times), self.n_params)
		if self.series_kernels.shape != expected:
			raise ValueError("Wrong shape of kernels. Anticipated ({0},{1}), but got {2}".format(expected[0], expected[1], self.series_kernels.shape))
		good = np.isfinite(times) & np.all(np.isfinite(kernels), axis=1)
		# the fill values are the first and last kernels of the series as given, finite or not
		self._interpolator = interp1d(times[good], kernels[good, :], axis=0, assume_sorted=True, bounds_error=False,
			fill_value=(kernels[0, :], kernels[-1, :]))
		# what the device entries read: the finite series and the two fill kernels in float64 (uploaded on first use, device_series)
		self._series_good = tuple(np.ascontiguousarray(a, dtype='float64') for a in (times[good], kernels[good, :], kernels[0, :], kernels[-1, :]))
		self._d_loaded = None

	def interpolate(self, time, xy):
		"""The change of the positions ``xy`` at ``time`` from the loaded series (image_motion.py:338-399)."""
		if self.warpmode == 'wcs':
			self._wcs_needs_series()
			k1, k2, dt, dx = self._wcs_frame_pairs(np.atleast_1d(np.asarray(time, dtype='float64')))
			xy = np.atleast_2d(xy)
			frames = [int(k1[0])] + ([int(k2[0])] if k2[0] >= 0 else [])
			j = self._wcs_jitters([self.series_kernels[k] for k in frames], xy)
			if k2[0] < 0:
				return j[0]
			# interp1d between the two frames (image_motion.py:383-389): slope * (time - t1) + jitter_1
			return (j[1] - j[0]) / dt[0] * dx[0] + j[0]
		if self._interpolator is None:
			raise ValueError("Interpolator is not defined. ")
		with warnings.catch_warnings():
			warnings.filterwarnings('ignore', category=RuntimeWarning, module='scipy')
			kernel = self._interpolator(time)
		return self.apply_kernel(xy, kernel)

	def jitter(self, time, column, row):
		"""(T, 2) changes in column and row of the position (column, row) at the timestamps ``time`` (image_motion.py:402-421)."""
		xy = np.array([column, row])
		if self.warpmode == 'wcs':
			return self._wcs_jitter(np.asarray(time, dtype='float64'), xy)
		out = np.empty((len(time), 2), dtype='float64')
		for k, t in enumerate(time):
			out[k, :] = self.interpolate(t, xy)
		return out

	def device_series(self, ctx=None):
		"""
		The loaded series on the device, uploaded once per ``load_series``: ``(code, S, d_times, d_kernels, d_first, d_last)``, the
		leading arguments of ``tp_motion_interpolate`` / ``tp_motion_star_positions`` (finite series, fill kernels as given).
		"""
		if self.warpmode not in WARPMODE_CODE:
			raise ValueError(f"no kernel series on the device for warpmode '{self.warpmode}'")
		if self._series_good is None:
			raise ValueError("Interpolator is not defined. ")
		ctx = self._context() if ctx is None else ctx
		if self._d_loaded is None or self._d_loaded[0] is not ctx:
			# (an 'unchanged' series has no parameters: one unread value stands in for the empty arrays)
			self._d_loaded = (ctx,) + tuple(ctx.array(a if a.size else np.zeros(1)) for a in self._series_good)
		return (WARPMODE_CODE[self.warpmode], len(self._series_good[0])) + self._d_loaded[1:]

	def interpolate_many(self, time, ctx=None):
		"""``(T, n_params)`` float64 kernels of the loaded series at the timestamps ``time`` (``tp_motion_interpolate``): the values
		``interpolate`` applies, bit for bit."""
		ctx = self._context() if ctx is None else ctx
		code, S, d_t, d_k, d_f, d_l = self.device_series(ctx)
		time = np.ascontiguousarray(np.atleast_1d(time), dtype='float64')
		T = len(time)
		out = ctx.empty((max(T, 1), max(self.n_params, 1)), 'float64')
		d_q = ctx.array(time)
		ctx._check(ctx.lib.tp_motion_interpolate(ctx.handle, code, S, d_t.ptr, d_k.ptr, d_f.ptr, d_l.ptr, T, d_q.ptr, out.ptr))
		return out.to_host()[:T, :self.n_params]

	def star_positions(self, time, xy, base_col=None, base_row=None, out_index=None, n_out=0, pitch=None, single=False, want_jitter=False,
		ctx=None, pos=None):
		"""
		``tp_motion_star_positions``: the positions ``xy`` ``(n, 2)`` (CCD column, row) under the loaded series at the timestamps
		``time``.  Returns ``(pos_col, pos_row, jitter)``: float64 DeviceArrays ``(n_out, pitch)`` holding
		float64(float32(base + jitter)) for the rows with ``out_index >= 0`` (None with ``n_out = 0``) and, with ``want_jitter``, the
		float64 jitter ``(n, T, 2)`` (else None).  ``single``: the float32 arithmetic ``apply_kernel`` does for float32 positions --
		what ``catalog_attime`` computes from the float32 catalogue.  ``pos``: a pair of DeviceArrays to write into instead of new ones.
		"""
		ctx = self._context() if ctx is None else ctx
		code, S, d_t, d_k, d_f, d_l = self.device_series(ctx)
		time = np.ascontiguousarray(np.atleast_1d(time), dtype='float64')
		xy = np.ascontiguousarray(xy, dtype='float64').reshape(-1, 2)
		n, T = len(xy), len(time)
		pitch = max(T, 1) if pitch is None else int(pitch)
		n_out = int(n_out)
		keep = [ctx.array(time), ctx.array(xy)]
		p_bc = p_br = p_oi = p_pc = p_pr = p_j = None
		pos_col = pos_row = jit = None
		if n_out > 0:
			out_index = np.ascontiguousarray(out_index, dtype='int64')
			if len(out_index) != n or np.any(out_index >= n_out):
				raise ValueError("out_index: one entry < n_out per position expected")
			base_col, base_row = np.ascontiguousarray(base_col, dtype='float32'), np.ascontiguousarray(base_row, dtype='float32')
			if base_col.shape != (n,) or base_row.shape != (n,):
				raise ValueError("base_col / base_row: one float32 value per position expected")
			if pos is not None and any(tuple(a.shape) != (n_out, pitch) or np.dtype(a.dtype) != np.dtype('float64') for a in pos):
				raise ValueError("pos: two float64 DeviceArrays (n_out, pitch) expected")
			keep += [ctx.array(base_col), ctx.array(base_row), ctx.array(out_index)]
			p_bc, p_br, p_oi = keep[2].ptr, keep[3].ptr, keep[4].ptr
			pos_col, pos_row = pos if pos is not None else (ctx.empty((n_out, pitch), 'float64'), ctx.empty((n_out, pitch), 'float64'))
			p_pc, p_pr = pos_col.ptr, pos_row.ptr
		if want_jitter:
			jit = ctx.empty((max(n, 1), max(T, 1), 2), 'float64')
			p_j = jit.ptr
		ctx._check(ctx.lib.tp_motion_star_positions(ctx.handle, code, S, d_t.ptr, d_k.ptr, d_f.ptr, d_l.ptr, T, keep[0].ptr, n, keep[1].ptr, int(bool(single)),
			p_bc, p_br, p_oi, n_out, p_pc, p_pr, pitch, p_j))
		return pos_col, pos_row, jit

	def jitter_many(self, time, columns, rows):
		"""
		``jitter(time, column, row)`` of many positions at once: a float64 DeviceArray ``(N, T, 2)`` of the changes in column and row
		(``tp_motion_star_positions``; for ``'wcs'`` the device path of ``jitter`` with every position a batch of its own).
		"""
		time = np.asarray(time, dtype='float64')
		xy = np.column_stack((np.asarray(columns, dtype='float64').ravel(), np.asarray(rows, dtype='float64').ravel()))
		if self.warpmode == 'wcs':
			return self._context().array(self._wcs_jitter_many(time, xy))
		if len(xy) == 0 or len(time) == 0:
			self.device_series()
			return self._context().zeros((len(xy), len(time), 2), 'float64')
		return self.star_positions(time, xy, want_jitter=True)[2]


	# -- warpmode 'wcs' ---------------------------------------------------------------------------------------------------
	def _wcs_needs_series(self):
		if self.wcs_ref is None:
			_no_wcs()
		if not getattr(self, '_wcs_loaded', False):
			raise ValueError("Interpolator is not defined. ")

	def _wcs_jitters(self, kernels, xy, d_params=None):
		"""(len(kernels), n, 2): all_world2pix(ref.all_pix2world(xy, 0), 0, maxiter=50, quiet=True) - xy per kernel, one launch."""
		if self.wcs_ref is None:
			_no_wcs()
		from . import wcs as wcsmod
		ctx = self._context()
		xy = np.atleast_2d(np.asarray(xy, dtype='float64'))
		if d_params is None:
			d_params = ctx.array(wcsmod.pack([wcsmod.as_wcs(k) for k in kernels]))
		d_cos = wcsmod.world_directions(ctx, self.wcs_ref, xy)
		pix, _, _ = wcsmod.world2pix_frames(ctx, d_params, len(kernels), d_cos, len(xy), np.array([0, len(xy)], dtype='int64'), 0, 1, 1e-4, 50)
		return pix - xy[None]

	def _wcs_load_series(self, times, kernels):
		"""image_motion.py:278-313: blank headers dropped, then every frame whose first footprint corner does not come back through
		all_world2pix(maxiter=50) (one device launch for the whole series)."""
		if self.wcs_ref is None:
			_no_wcs()
		from . import wcs as wcsmod
		if len(kernels) != len(times):
			raise ValueError("Wrong shape of kernels.")
		times = np.asarray(times, dtype='float64')
		good = np.ones(len(times), dtype='bool')
		parsed = []
		for k, h in enumerate(kernels):
			if isinstance(h, str) and not h.strip():
				good[k] = False
				continue
			parsed.append(wcsmod.as_wcs(h))
		ctx = self._context()
		d_params = ctx.array(wcsmod.pack(parsed)) if parsed else None
		if parsed:
			ok = wcsmod.footprint_check(ctx, d_params, len(parsed)) == 0
			idx = np.flatnonzero(good)
			good[idx[~ok]] = False
			parsed = [w for w, o in zip(parsed, ok) if o]
			d_params = ctx.array(wcsmod.pack(parsed)) if parsed else None
		self.series_times = times[good]
		self.series_kernels = parsed
		self._d_series = d_params
		self._wcs_loaded = True

	def _wcs_frame_pairs(self, t):
		"""Per time: (k1, k2, t2 - t1, t - t1) of image_motion.py:357-389 (k2 = -1: frame k1's jitter alone)."""
		st = self.series_times
		if len(st) == 0:
			raise ValueError("Timestamp outside timeseries interval")
		k1 = np.empty(len(t), dtype='int32')
		k2 = np.full(len(t), -1, dtype='int32')
		out = (t < st[0]) | (t > st[-1])
		if np.any(out):
			with np.errstate(invalid='ignore'):
				dt = np.median(np.diff(st)) if len(st) > 1 else np.nan
			first = np.abs(t - st[0]) < dt
			last = ~first & (np.abs(t - st[-1]) < dt)
			if np.any(out & ~first & ~last):
				raise ValueError("Timestamp outside timeseries interval")
			k1[out & first] = 0
			k1[out & last] = len(st) - 1
		if np.any(~np.isfinite(t)):
			raise ValueError("Timestamp outside timeseries interval")
		inn = ~out
		k = np.searchsorted(st, t[inn], side='right')
		k1[inn] = k - 1
		miss = st[k - 1] != t[inn]
		k2i = np.where(miss, k, -1)
		k2[inn] = k2i
		t1 = st[k1]
		t2 = np.where(k2 >= 0, st[np.maximum(k2, 0)], t1)
		return k1, k2, t2 - t1, t - t1

	def _wcs_jitter_many(self, time, xy):
		"""(N, T, 2): ``_wcs_jitter`` of every position, each a batch of its own (the iteration's stopping test is taken per batch)."""
		self._wcs_needs_series()
		from . import wcs as wcsmod
		k1, k2, dt, dx = self._wcs_frame_pairs(time)
		ctx = self._context()
		n = len(xy)
		d_cos = wcsmod.world_directions(ctx, self.wcs_ref, xy)
		pix, _, _ = wcsmod.world2pix_frames(ctx, self._d_series, len(self.series_kernels), d_cos, n, np.arange(n + 1, dtype='int64'), 0, 1, 1e-4, 50)
		j = np.moveaxis(pix - xy[None], 0, 1)    # (N, F, 2)
		out = j[:, k1].copy()
		two = k2 >= 0
		if np.any(two):
			j1, j2 = j[:, k1[two]], j[:, k2[two]]
			out[:, two] = (j2 - j1) / dt[None, two, None] * dx[None, two, None] + j1
		return out

	def _wcs_jitter(self, time, xy):
		self._wcs_needs_series()
		k1, k2, dt, dx = self._wcs_frame_pairs(time)
		j = self._wcs_jitters(self.series_kernels, xy, d_params=self._d_series)[:, 0, :]    # (F, 2)
		out = j[k1].copy()
		two = k2 >= 0
		if np.any(two):
			j1, j2 = j[k1[two]], j[k2[two]]
			out[two] = (j2 - j1) / dt[two, None] * dx[two, None] + j1
		return out


def movement_from_header(header, times=None):
	"""
	A :class:`MovementKernel` with its series loaded from a ``.tpstack`` header (``frameio.read_header``) that carries the
	``movement_kernel`` of the prepare stage (``attrs['movement_kernel']``: ``kernels``, ``warpmode``, ``ref_frame``) -- what
	``BasePhotometry.MovementKernel`` builds from the HDF5 dataset (BasePhotometry.py:1185-1221).  ``times``: the timestamps of
	the series (default: the header's ``time`` vector).  A header with per-frame WCS headers (``attrs['wcs_headers']``, written by
	``frameio.write_stack(wcs_headers=...)``) gives a ``'wcs'`` kernel instead.  Returns None when the header holds no kernels.
	"""
	attrs = header.get('attrs') or {}
	if attrs.get('wcs_headers') is not None:
		# per-frame WCS headers win, as in BasePhotometry.py:1185-1221
		times = np.asarray(header['time'] if times is None else times, dtype='float64')
		m = MovementKernel(warpmode='wcs', wcs_ref=attrs['wcs_ref'])
		m.load_series(times, list(attrs['wcs_headers']))
		m.ref_frame = None
		return m
	mk = attrs.get('movement_kernel')
	if mk is None:
		return None
	kernels = np.asarray(mk['kernels'], dtype='float64')
	times = np.asarray(header['time'] if times is None else times, dtype='float64')
	m = MovementKernel(warpmode=mk['warpmode'])
	m.load_series(times, kernels.reshape(len(times), m.n_params))
	m.ref_frame = None if mk.get('ref_frame') is None else int(mk['ref_frame'])
	return m
