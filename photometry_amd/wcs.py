# -*- coding: utf-8 -*-
"""
TAN-SIP world coordinate systems on the device: what ``ImageMovementKernel(warpmode='wcs')`` (image_motion.py:113-421) asks of
``astropy.wcs.WCS`` -- ``all_pix2world`` and astropy 4.3's ``all_world2pix`` iteration -- for the celestial TAN projection with
or without SIP distortion, the WCS of TESS FFIs.

:meth:`TanSipWCS.from_header` parses FITS header cards (80-column card strings as ``fits.Header.fromstring`` reads them,
newline-separated cards, or a dict) and packs one float64 parameter block (``TP_WCS_PARAMS`` values) for the device: the native to
celestial rotation of CRVAL / LONPOLE, CRPIX, CD and its inverse, the SIP A / B coefficients.  Every transform runs in
csrc/wcs.hip; there is no CPU path.  Anything outside that model (another projection, PV terms, lookup-table distortions, more
axes, a singular CD) raises ``ValueError`` naming the keyword.  DESIGN.md section 11 defines the batch rule of ``all_world2pix``
and the deliberate differences from astropy; tests/wcs_common.py restates the transforms in spherical trigonometry.
"""

import re
import numpy as np

#: the parameter block of one frame (include/tessphot_hip.h)
N_PARAMS = 224
MAX_SIP_ORDER = 9
#: status bits of world -> pixel (TP_WCS_*)
DIVERGENT, SLOW, INVALID, SCHEDULE = 1, 2, 4, 8

_CARD = re.compile(r"^([A-Z0-9_-]{1,8})\s*=\s?(.*)$")
_NUM = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)([EeDd][+-]?\d+)?$")
# WCS keywords of an alternate description (a letter after the primary keyword: CTYPE1P, WCSNAMEP, CD1_1A, ...)
_ALT = re.compile(r"^(WCSNAME|WCSAXES|CTYPE\d|CUNIT\d|CRPIX\d|CRVAL\d|CDELT\d|CROTA\d|CD\d_\d|PC\d_\d|PV\d_\d+|PS\d_\d+|LONPOLE|LATPOLE|"
	r"RADESYS|EQUINOX|CNAME\d|CRDER\d|CSYER\d|MJDREF|DATEREF)[A-Z]$")
# (A_DMAX / B_DMAX only record the largest SIP distortion: astropy and wcslib ignore them, and so does this parser)
_REFUSED = re.compile(r"^(PV\d_\d+|PS\d_\d+|CPDIS\d|CPERR\d|CQDIS\d|D2IMDIS\d|D2IMERR\d|D2IMEXT|D2IM\d|DP\d|DQ\d|CROTA\d)$")


class NoConvergence(Exception):
	"""``all_world2pix`` did not converge for some points (astropy.wcs.NoConvergence): ``best_solution``, ``divergent``, ``slow_conv``."""

	def __init__(self, message, best_solution=None, divergent=None, slow_conv=None, niter=None):
		super().__init__(message)
		self.best_solution = best_solution
		self.divergent = divergent
		self.slow_conv = slow_conv
		self.niter = niter


def _value(text):
	"""The value of a card's value field (after '= '): string, bool, int or float (a ``D`` exponent allowed)."""
	t = text.strip()
	if t.startswith("'"):
		out, i = [], 1
		while i < len(t):
			if t[i] == "'":
				if i + 1 < len(t) and t[i + 1] == "'":
					out.append("'")
					i += 2
					continue
				break
			out.append(t[i])
			i += 1
		return ''.join(out).rstrip()
	t = t.split('/', 1)[0].strip()
	if t in ('T', 'F'):
		return t == 'T'
	if _NUM.match(t):
		if re.match(r"^[+-]?\d+$", t):
			return int(t)
		return float(t.replace('D', 'E').replace('d', 'e'))
	return t


def parse_cards(header):
	"""``{keyword: value}`` of a header string (80-column cards, or one card per line) or a dict (values or (value, comment))."""
	if isinstance(header, dict):
		return {str(k).upper(): (v[0] if isinstance(v, tuple) else v) for k, v in header.items()}
	if not isinstance(header, str):
		raise TypeError("header: a string of FITS cards or a dict expected")
	if '\n' in header:
		cards = header.splitlines()
	else:
		cards = [header[i:i + 80] for i in range(0, len(header), 80)]
	out = {}
	for card in cards:
		key = card[:8].strip()
		if key in ('', 'COMMENT', 'HISTORY', 'CONTINUE'):
			continue
		if key == 'END':
			break
		m = _CARD.match(card.rstrip()) if card[8:10] != '= ' else None
		if card[8:10] == '= ':
			out[key] = _value(card[10:])
		elif m:
			out[m.group(1)] = _value(m.group(2))
	return out


def _sincosd(deg):
	"""sin and cos of an angle in degrees, exact at multiples of 90 (as wcslib's sind / cosd)."""
	deg = float(deg)
	r = deg % 90.0
	if r == 0.0:
		q = int(round(deg / 90.0)) % 4
		return ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0))[q]
	a = np.deg2rad(deg)
	return float(np.sin(a)), float(np.cos(a))


def rotation_matrix(crval1, crval2, lonpole):
	"""The native -> celestial rotation c = M n of a zenithal projection (Calabretta & Greisen 2002, eq. 2, as a matrix)."""
	sa, ca = _sincosd(crval1)
	sd, cd = _sincosd(crval2)
	sp, cp = _sincosd(lonpole)
	X = np.array([-sd * cp, -sd * sp, cd])      # cos(dec) cos(ra - ra_p)
	Y = np.array([sp, -cp, 0.0])                # cos(dec) sin(ra - ra_p)
	Z = np.array([cd * cp, cd * sp, sd])        # sin(dec)
	return np.array([ca * X - sa * Y, sa * X + ca * Y, Z])


def _sip_matrix(cards, name, order):
	m = np.zeros((10, 10))
	for p in range(order + 1):
		for q in range(order + 1 - p):
			m[p, q] = float(cards.get(f'{name}_{p}_{q}', 0.0))
	for k in cards:
		mm = re.match(rf'^{name}_(\d+)_(\d+)$', k)
		if mm and int(mm.group(1)) + int(mm.group(2)) > order:
			raise ValueError(f"{k}: SIP term above {name}_ORDER = {order}")
	return m


class TanSipWCS(object):
	"""
	A celestial TAN (optionally TAN-SIP) WCS, with astropy.wcs.WCS's transforms running on the device.

	Methods take astropy's arguments -- an ``(N, 2)`` array and ``origin``, or ``x, y, origin`` (then a pair of arrays is
	returned) -- and return float64.  ``all_world2pix`` takes the points of one call as one batch, as astropy does.
	"""

	def __init__(self, crpix, crval, cd, lonpole=None, latpole=None, a=None, b=None, ap=None, bp=None, ctx=None, naxis=None):
		self.crpix = np.array(crpix, dtype='float64')
		self.crval = np.array(crval, dtype='float64')
		self.cd = np.array(cd, dtype='float64').reshape(2, 2)
		det = self.cd[0, 0] * self.cd[1, 1] - self.cd[0, 1] * self.cd[1, 0]
		if not np.isfinite(det) or det == 0.0:
			raise ValueError("CD: singular linear transformation matrix")
		self.lonpole = float(lonpole) if lonpole is not None else (180.0 if self.crval[1] < 90.0 else 0.0)
		self.latpole = 90.0 if latpole is None else float(latpole)
		self.a, self.b = a, b            # (order, 10 x 10) or None
		self.ap, self.bp = ap, bp        # parsed, not used (astropy's all_world2pix does not use them either)
		self.naxis = naxis
		self.ctx = ctx
		self._d_params = None

	@property
	def has_sip(self):
		return self.a is not None

	@classmethod
	def from_header(cls, header, ctx=None):
		"""Parse a header (card string, newline-separated cards, or a dict); ``ValueError`` naming the keyword outside TAN-SIP."""
		if isinstance(header, TanSipWCS):
			return header
		cards = parse_cards(header)
		cards = {k: v for k, v in cards.items() if not _ALT.match(k)}
		for k in cards:
			if _REFUSED.match(k):
				raise ValueError(f"{k}: not supported (TAN and TAN-SIP only)")
			m = re.match(r'^(CTYPE|CRPIX|CRVAL|CDELT|CUNIT)(\d+)$', k) or re.match(r'^(CD|PC)(\d+)_(\d+)$', k)
			if m and any(int(g) > 2 for g in m.groups()[1:]):
				raise ValueError(f"{k}: more than two axes")
		if int(cards.get('WCSAXES', 2)) != 2:
			raise ValueError("WCSAXES: two celestial axes expected")
		ct1, ct2 = str(cards.get('CTYPE1', '')).strip(), str(cards.get('CTYPE2', '')).strip()
		if ct1 not in ('RA---TAN', 'RA---TAN-SIP'):
			raise ValueError(f"CTYPE1: '{ct1}' not supported (RA---TAN or RA---TAN-SIP)")
		if ct2 not in ('DEC--TAN', 'DEC--TAN-SIP'):
			raise ValueError(f"CTYPE2: '{ct2}' not supported (DEC--TAN or DEC--TAN-SIP)")
		for k in ('CUNIT1', 'CUNIT2'):
			if k in cards and str(cards[k]).strip() not in ('', 'deg'):
				raise ValueError(f"{k}: '{cards[k]}' not supported (deg)")
		crpix = [float(cards.get('CRPIX1', 0.0)), float(cards.get('CRPIX2', 0.0))]
		crval = [float(cards.get('CRVAL1', 0.0)), float(cards.get('CRVAL2', 0.0))]
		has_pc = any(re.match(r'^PC\d_\d$', k) for k in cards)
		has_cd = any(re.match(r'^CD\d_\d$', k) for k in cards)
		if has_cd and not has_pc:
			cd = [[float(cards.get(f'CD{i}_{j}', 0.0)) for j in (1, 2)] for i in (1, 2)]
		else:
			# wcslib: PCi_j (default the unit matrix) scaled by CDELTi, PC taking precedence over CD
			pc = [[float(cards.get(f'PC{i}_{j}', 1.0 if i == j else 0.0)) for j in (1, 2)] for i in (1, 2)]
			cdelt = [float(cards.get('CDELT1', 1.0)), float(cards.get('CDELT2', 1.0))]
			cd = [[cdelt[i] * pc[i][j] for j in range(2)] for i in range(2)]
		cdm = np.array(cd)
		det = cdm[0, 0] * cdm[1, 1] - cdm[0, 1] * cdm[1, 0]
		if not np.isfinite(det) or det == 0.0:
			raise ValueError(("PC" if has_pc else "CD") + ": singular linear transformation matrix")
		a = b = ap = bp = None
		if 'A_ORDER' in cards or 'B_ORDER' in cards:
			for k in ('A_ORDER', 'B_ORDER'):
				if k not in cards:
					raise ValueError(f"{k}: missing (SIP needs A_ORDER and B_ORDER)")
				if not 0 <= int(cards[k]) <= MAX_SIP_ORDER:
					raise ValueError(f"{k}: {cards[k]} outside 0 .. {MAX_SIP_ORDER}")
			a = (int(cards['A_ORDER']), _sip_matrix(cards, 'A', int(cards['A_ORDER'])))
			b = (int(cards['B_ORDER']), _sip_matrix(cards, 'B', int(cards['B_ORDER'])))
			if 'AP_ORDER' in cards:
				ap = (int(cards['AP_ORDER']), _sip_matrix(cards, 'AP', int(cards['AP_ORDER'])))
			if 'BP_ORDER' in cards:
				bp = (int(cards['BP_ORDER']), _sip_matrix(cards, 'BP', int(cards['BP_ORDER'])))
		naxis = (int(cards['NAXIS1']), int(cards['NAXIS2'])) if 'NAXIS1' in cards and 'NAXIS2' in cards else None
		return cls(crpix, crval, cd, lonpole=cards.get('LONPOLE'), latpole=cards.get('LATPOLE'), a=a, b=b, ap=ap, bp=bp, ctx=ctx, naxis=naxis)

	def params(self):
		"""The packed float64 parameter block of this WCS (the layout of include/tessphot_hip.h)."""
		p = np.zeros(N_PARAMS)
		p[0:9] = rotation_matrix(self.crval[0], self.crval[1], self.lonpole).ravel()
		p[9:11] = self.crpix
		p[11:15] = self.cd.ravel()
		c = self.cd
		det = c[0, 0] * c[1, 1] - c[0, 1] * c[1, 0]
		p[15:19] = [c[1, 1] / det, -c[0, 1] / det, -c[1, 0] / det, c[0, 0] / det]
		if self.has_sip:
			p[19], p[20], p[21] = self.a[0], self.b[0], 1.0
			p[24:124] = self.a[1].ravel()
			p[124:224] = self.b[1].ravel()
		return p

	# -- device plumbing -------------------------------------------------------------------------------------------------
	def _context(self):
		if self.ctx is None:
			from .device import Context
			self.ctx = Context(0)
		return self.ctx

	def _dparams(self):
		if self._d_params is None:
			self._d_params = self._context().array(self.params())
		return self._d_params

	@staticmethod
	def _points(args, what):
		"""(N, 2) float64 points and origin from astropy-style arguments; ``pair``: the caller gave x, y separately."""
		if len(args) == 2:
			xy = np.asarray(args[0], dtype='float64')
			if xy.ndim != 2 or xy.shape[1] != 2:
				raise ValueError(f"{what}: an (N, 2) array expected")
			return np.ascontiguousarray(xy), int(args[1]), None
		if len(args) == 3:
			x, y = np.broadcast_arrays(np.asarray(args[0], dtype='float64'), np.asarray(args[1], dtype='float64'))
			return np.ascontiguousarray(np.column_stack((x.ravel(), y.ravel()))), int(args[2]), x.shape
		raise TypeError(f"{what}: expected (xy, origin) or (x, y, origin)")

	@staticmethod
	def _ret(out, shape):
		return out if shape is None else (out[:, 0].reshape(shape), out[:, 1].reshape(shape))

	def _pix2world(self, args, mode, what):
		xy, origin, shape = self._points(args, what)
		if origin not in (0, 1):
			raise ValueError("origin: 0 or 1")
		ctx = self._context()
		n = len(xy)
		d_xy, d_out = ctx.array(xy if n else np.zeros((1, 2))), ctx.empty((max(n, 1), 2), 'float64')
		ctx._check(ctx.lib.tp_wcs_pix2world(ctx.handle, self._dparams().ptr, n, d_xy.ptr, origin, mode, d_out.ptr, None))
		return self._ret(d_out.to_host()[:n], shape)

	def pix2foc(self, *args):
		"""SIP distortion of pixel coordinates (no SIP: the pixels themselves)."""
		return self._pix2world(args, 0, 'pix2foc')

	def wcs_pix2world(self, *args, **kwargs):
		"""Pixel -> (ra, dec) degrees without SIP."""
		return self._pix2world(args, 1, 'wcs_pix2world')

	def all_pix2world(self, *args, **kwargs):
		"""Pixel -> (ra, dec) degrees: pix2foc, CD, TAN, the sky rotation (ra in [0, 360))."""
		return self._pix2world(args, 2, 'all_pix2world')

	def _world2pix(self, args, all_, tolerance, maxiter, quiet, what):
		radec, origin, shape = self._points(args, what)
		if origin not in (0, 1):
			raise ValueError("origin: 0 or 1")
		ctx = self._context()
		n = len(radec)
		d_radec = ctx.array(radec if n else np.zeros((1, 2)))
		d_cos = ctx.empty((max(n, 1), 3), 'float64')
		ctx._check(ctx.lib.tp_wcs_radec(ctx.handle, n, d_radec.ptr, d_cos.ptr))
		pix, status, iters = world2pix_frames(ctx, self._dparams(), 1, d_cos, n, np.array([0, n], dtype='int64'), origin, all_, tolerance, maxiter)
		pix, status = pix[0], status[0]
		self.last_iterations = int(iters[0, 0])
		self.last_status = status
		if all_ and not quiet and np.any(status & (DIVERGENT | SLOW)):
			div = np.flatnonzero(status & DIVERGENT)
			slow = np.flatnonzero(status & SLOW)
			raise NoConvergence("'WCS.all_world2pix' failed to converge to the requested accuracy after {:d} iterations.".format(self.last_iterations),
				best_solution=pix, divergent=div if len(div) else None, slow_conv=slow if len(slow) else None, niter=self.last_iterations)
		return self._ret(pix, shape)

	def wcs_world2pix(self, *args, **kwargs):
		"""(ra, dec) degrees -> pixel without SIP."""
		return self._world2pix(args, 0, 1e-4, 1, True, 'wcs_world2pix')

	def all_world2pix(self, *args, tolerance=1e-4, maxiter=20, quiet=False, **kwargs):
		"""(ra, dec) degrees -> pixel: astropy 4.3's fixed-point iteration over the points of the call as one batch."""
		return self._world2pix(args, 1, float(tolerance), int(maxiter), quiet, 'all_world2pix')

	def calc_footprint(self, axes=None):
		"""The four corners (1, 1), (1, n2), (n1, n2), (n1, 1) (FITS pixels) in (ra, dec) degrees (astropy's undistorted=True)."""
		if axes is None:
			if self.naxis is None:
				raise ValueError("calc_footprint: axes needed (no NAXIS1 / NAXIS2 in the header)")
			axes = self.naxis
		n1, n2 = axes
		corners = np.array([[1, 1], [1, n2], [n1, n2], [n1, 1]], dtype='float64')
		return self.all_pix2world(corners, 1)


def as_wcs(obj, ctx=None):
	"""A :class:`TanSipWCS` from a header string, a card dict or a TanSipWCS."""
	if isinstance(obj, TanSipWCS):
		if ctx is not None and obj.ctx is None:
			obj.ctx = ctx
		return obj
	return TanSipWCS.from_header(obj, ctx=ctx)


def pack(wcs_list):
	"""(F, N_PARAMS) float64 parameter blocks of a list of :class:`TanSipWCS`."""
	return np.ascontiguousarray(np.stack([w.params() for w in wcs_list])) if len(wcs_list) else np.zeros((0, N_PARAMS))


def _check_offsets(offsets, n):
	offsets = np.ascontiguousarray(offsets, dtype='int64')
	if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] < 0 or offsets[-1] > n or np.any(np.diff(offsets) < 0):
		raise ValueError("batch offsets must rise from >= 0 to <= the number of points")
	return offsets


def world2pix_frames(ctx, d_params, n_frames, d_cos, n, offsets, origin=0, all_=1, tolerance=1e-4, maxiter=20):
	"""
	``tp_wcs_world2pix``: the ``n`` world directions ``d_cos`` (device (n, 3)) in each of ``n_frames`` frames (device parameter
	blocks), batches at ``offsets``.  Returns host arrays ``pix`` (F, n, 2), ``status`` (F, n) and ``iters`` (F, n_batches).
	"""
	offsets = _check_offsets(offsets, n)
	nb = len(offsets) - 1
	d_pix = ctx.empty((max(n_frames, 1), max(n, 1), 2), 'float64')
	d_st = ctx.empty((max(n_frames, 1), max(n, 1)), 'int32')
	d_it = ctx.empty((max(n_frames, 1), max(nb, 1)), 'int32')
	ctx._check(ctx.lib.tp_wcs_world2pix(ctx.handle, d_params.ptr, int(n_frames), int(n), nb, offsets.ctypes.data, d_cos.ptr, int(origin), int(all_),
		float(tolerance), int(maxiter), d_pix.ptr, d_st.ptr, d_it.ptr))
	return (d_pix.to_host()[:n_frames, :n], d_st.to_host()[:n_frames, :n], d_it.to_host()[:n_frames, :nb])


def world_directions(ctx, ref, xy):
	"""Device (n, 3) celestial unit vectors of the 0-based pixels ``xy`` (n, 2) under the WCS ``ref`` (all_pix2world)."""
	xy = np.ascontiguousarray(xy, dtype='float64').reshape(-1, 2)
	n = len(xy)
	d_xy = ctx.array(xy if n else np.zeros((1, 2)))
	d_cos = ctx.empty((max(n, 1), 3), 'float64')
	d_ref = ctx.array(ref.params())
	ctx._check(ctx.lib.tp_wcs_pix2world(ctx.handle, d_ref.ptr, n, d_xy.ptr, 0, 2, None, d_cos.ptr))
	ctx.sync()
	return d_cos


def footprint_check(ctx, d_params, n_frames, tolerance=1e-4, maxiter=50):
	"""``tp_wcs_footprint_check``: status bits per frame (0: ``load_series`` keeps the frame)."""
	d_st = ctx.empty((max(n_frames, 1),), 'int32')
	ctx._check(ctx.lib.tp_wcs_footprint_check(ctx.handle, d_params.ptr, int(n_frames), float(tolerance), int(maxiter), d_st.ptr))
	return d_st.to_host()[:n_frames]


def star_positions(ctx, d_params, n_frames, ref, offsets, xy32, base_col, base_row, out_index, n_out, k1, k2, dt, dx, tolerance=1e-4, maxiter=50):
	"""
	``tp_wcs_star_positions``: float64 DeviceArrays ``(pos_col, pos_row)`` of shape (n_out, T) -- float64(float32(base + jitter))
	per catalogue row with ``out_index >= 0`` and cadence -- and the host status bits per row (OR over the cadences).
	"""
	xy32 = np.ascontiguousarray(xy32, dtype='float32').reshape(-1, 2)
	n = len(xy32)
	offsets = _check_offsets(offsets, n)
	out_index = np.ascontiguousarray(out_index, dtype='int64')
	if len(out_index) != n or np.any(out_index >= n_out):
		raise ValueError("out_index: one entry < n_out per row expected")
	k1 = np.ascontiguousarray(k1, dtype='int32')
	k2 = np.ascontiguousarray(k2, dtype='int32')
	T = len(k1)
	if np.any((k1 < 0) | (k1 >= n_frames)) or np.any((k2 < -1) | (k2 >= n_frames)):
		raise ValueError("frame indices outside the series")
	keep = [ctx.array(a if len(a) else np.zeros(1, a.dtype)) for a in (xy32, np.ascontiguousarray(base_col, dtype='float32'),
		np.ascontiguousarray(base_row, dtype='float32'), out_index, k1, k2, np.ascontiguousarray(dt, dtype='float64'),
		np.ascontiguousarray(dx, dtype='float64'), ref.params())]
	d_xy, d_bc, d_br, d_oi, d_k1, d_k2, d_dt, d_dx, d_ref = keep
	pos_col = ctx.empty((max(n_out, 1), max(T, 1)), 'float64')
	pos_row = ctx.empty((max(n_out, 1), max(T, 1)), 'float64')
	d_st = ctx.zeros((max(n, 1),), 'int32')
	ctx._check(ctx.lib.tp_wcs_star_positions(ctx.handle, d_params.ptr, int(n_frames), d_ref.ptr, n, len(offsets) - 1, offsets.ctypes.data, d_xy.ptr,
		d_bc.ptr, d_br.ptr, d_oi.ptr, int(n_out), T, d_k1.ptr, d_k2.ptr, d_dt.ptr, d_dx.ptr, float(tolerance), int(maxiter), pos_col.ptr, pos_row.ptr,
		max(T, 1), d_st.ptr))
	status = d_st.to_host()[:n]
	return pos_col, pos_row, status
