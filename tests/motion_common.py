# -*- coding: utf-8 -*-
"""
CPU restatement of the image-motion kernels (photometry/image_motion.py): the definition the device port
(``photometry_amd/csrc/motion.hip``) is held to.

* :func:`prepare_flux` -- ``ImageMovementKernel._prepare_flux`` (image_motion.py:74-110) in float32: log10 of the
  min-shifted flux, rescaled to [-1, 1], the Scharr gradient magnitude of scikit-image 0.19 (``mode='reflect'``, per axis
  ``[1, 0, -1]`` along the axis then ``[3, 10, 3] / 16`` across it, ``sqrt((h**2 + v**2) / 2)``), NaN -> 0.
* :func:`ecc` -- the forward-additive ECC maximisation of Evangelidis & Psarakis (IEEE TPAMI 30(10), 2008) in the sequence
  OpenCV's ``findTransformECC`` runs it (``gaussFiltSize=5``, all-ones input mask), written literally in the zero-mean form:
  the device computes the same quantities from raw moments, so the two check each other.

Deliberate differences from OpenCV: the bilinear warp interpolates continuously (no 1/32-px quantisation), the
small matrix algebra and the warp are float64, and every sum runs over the warped mask.
"""

import numpy as np
from scipy.ndimage import correlate1d

N_PARAMS = {'translation': 2, 'euclidian': 3, 'affine': 6}

#: frame states (``tp_motion_ecc``'s d_status)
ACTIVE, CONVERGED, CAP_REACHED, FAILED_NAN, FAILED_LAMBDA = 0, 1, 2, 3, 4

SCHARR_SMOOTH = np.array([3.0, 10.0, 3.0]) / 16.0
BLUR5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0     # OpenCV's fixed table for ksize 5, sigma 0
DIFF = np.array([-0.5, 0.0, 0.5])


def scharr(f1):
	"""skimage.filters.scharr(f1) with mask=None, mode='reflect', float32 kept."""
	f1 = np.asarray(f1, dtype='float32')
	h = correlate1d(correlate1d(f1, [1.0, 0.0, -1.0], axis=0, mode='reflect'), SCHARR_SMOOTH, axis=1, mode='reflect')
	v = correlate1d(correlate1d(f1, [1.0, 0.0, -1.0], axis=1, mode='reflect'), SCHARR_SMOOTH, axis=0, mode='reflect')
	out = h * h + v * v
	return np.sqrt(out / np.float32(2))


def prepare_flux(frame):
	"""image_motion.py:74-110 in float32."""
	flux = np.asarray(frame, dtype='float32')
	with np.errstate(invalid='ignore', divide='ignore'), _nan_quiet():
		flux = np.log10(flux - np.nanmin(flux) + np.float32(1.0))
		fmax = np.nanmax(flux)
		fmin = np.nanmin(flux)
		ran = np.abs(fmax - fmin)
		flux1 = np.float32(-1) + np.float32(2) * ((flux - fmin) / ran)
		flux1 = scharr(flux1)
	flux1[np.isnan(flux1)] = 0
	return np.asarray(flux1, dtype='float32')


class _nan_quiet(object):
	"""nanmin / nanmax of an all-NaN frame warn; the reference lets them."""
	def __enter__(self):
		import warnings
		self._w = warnings.catch_warnings()
		self._w.__enter__()
		warnings.simplefilter('ignore', RuntimeWarning)

	def __exit__(self, *args):
		self._w.__exit__(*args)


def blur5(img):
	"""GaussianBlur(ksize 5, sigma 0) with BORDER_REFLECT_101: rows first, then columns, float32 in between."""
	img = np.asarray(img, dtype='float32')
	return correlate1d(correlate1d(img, BLUR5, axis=1, mode='mirror'), BLUR5, axis=0, mode='mirror')


def gradients(blurred):
	"""filter2D with [-0.5, 0, 0.5] (and its transpose), BORDER_REFLECT_101, float32."""
	return correlate1d(blurred, DIFF, axis=1, mode='mirror'), correlate1d(blurred, DIFF, axis=0, mode='mirror')


def _bilinear(src, xs, ys):
	"""src(xs, ys) bilinear, constant 0 outside the frame (float64)."""
	R, C = src.shape
	x0 = np.floor(xs)
	y0 = np.floor(ys)
	fx = xs - x0
	fy = ys - y0
	x0 = x0.astype(np.int64)
	y0 = y0.astype(np.int64)
	s = src.astype('float64')

	def at(yy, xx):
		ok = (yy >= 0) & (yy < R) & (xx >= 0) & (xx < C)
		v = np.zeros(xx.shape)
		v[ok] = s[yy[ok], xx[ok]]
		return v
	a, b = at(y0, x0), at(y0, x0 + 1)
	c, d = at(y0 + 1, x0), at(y0 + 1, x0 + 1)
	return (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c + fx * d)


def warp_to_kernel(w, warpmode):
	"""calc_kernel's return value (image_motion.py:241-256) from the 2 x 3 warp."""
	if warpmode == 'affine':
		return w.flatten()
	if warpmode == 'euclidian':
		return np.array([w[0, 2], w[1, 2], np.arctan2(w[1, 0], w[0, 0])])
	return np.array([w[0, 2], w[1, 2]])


def ecc(template_prepared, image_prepared, warpmode, max_iter=10000, eps=1e-6):
	"""
	findTransformECC(template, input, eye(2, 3), mode, (EPS | COUNT, max_iter, eps), all-ones mask, gaussFiltSize=5).

	Returns ``(kernel, rho, iterations, status)``: ``kernel`` as calc_kernel returns it (NaN when the frame failed), ``rho``
	the last measured correlation, ``iterations`` the loop bodies run, ``status`` one of the frame states above.
	"""
	P = N_PARAMS[warpmode]
	T = blur5(template_prepared).astype('float64')
	B = blur5(image_prepared)
	gx, gy = gradients(B)
	R, C = B.shape
	yy, xx = np.mgrid[0:R, 0:C].astype('float64')
	w = np.eye(2, 3)
	rho, last_rho = -1.0, -eps
	i = 1
	status = ACTIVE
	while i <= max_iter and abs(rho - last_rho) >= eps:
		xs = w[0, 0] * xx + w[0, 1] * yy + w[0, 2]
		ys = w[1, 0] * xx + w[1, 1] * yy + w[1, 2]
		with np.errstate(invalid='ignore'):
			mask = (np.floor(xs + 0.5) >= 0) & (np.floor(xs + 0.5) <= C - 1) & (np.floor(ys + 0.5) >= 0) & (np.floor(ys + 0.5) <= R - 1)
		xm, ym = xs[mask], ys[mask]
		Iw = _bilinear(B, xm, ym)
		gxw = _bilinear(gx, xm, ym)
		gyw = _bilinear(gy, xm, ym)
		Tm = T[mask]
		N = mask.sum()
		with np.errstate(invalid='ignore', divide='ignore'), _nan_quiet():
			Iz = Iw - Iw.mean()
			Tz = Tm - Tm.mean()
			img_norm = np.sqrt(N) * Iw.std()
			tmp_norm = np.sqrt(N) * Tm.std()
		x, y = xx[mask], yy[mask]
		if warpmode == 'translation':
			J = np.stack([gxw, gyw])
		elif warpmode == 'euclidian':
			c, s = w[0, 0], w[1, 0]
			J = np.stack([gxw * (-x * s - y * c) + gyw * (x * c - y * s), gxw, gyw])
		else:
			J = np.stack([gxw * x, gyw * x, gxw * y, gyw * y, gxw, gyw])
		H = J @ J.T
		try:
			Hinv = np.linalg.inv(H)
		except np.linalg.LinAlgError:
			Hinv = np.zeros((P, P))
		corr = float(Tz @ Iz)
		last_rho = rho
		with np.errstate(invalid='ignore', divide='ignore'):
			rho = corr / (img_norm * tmp_norm)
		if np.isnan(rho):
			status = FAILED_NAN
			break
		pI = J @ Iz
		pT = J @ Tz
		hpI = Hinv @ pI
		lam_n = img_norm * img_norm - pI @ hpI
		lam_d = corr - pT @ hpI
		if lam_d <= 0.0:
			status = FAILED_LAMBDA
			break
		lam = lam_n / lam_d
		dp = Hinv @ (lam * pT - pI)
		if warpmode == 'translation':
			w[0, 2] += dp[0]
			w[1, 2] += dp[1]
		elif warpmode == 'euclidian':
			theta = dp[0] + np.arcsin(w[1, 0])
			w[0, 2] += dp[1]
			w[1, 2] += dp[2]
			w[0, 0] = w[1, 1] = np.cos(theta)
			w[1, 0] = np.sin(theta)
			w[0, 1] = -w[1, 0]
		else:
			w[0, 0] += dp[0]
			w[1, 0] += dp[1]
			w[0, 1] += dp[2]
			w[1, 1] += dp[3]
			w[0, 2] += dp[4]
			w[1, 2] += dp[5]
		i += 1
	iterations = i - 1 if status == ACTIVE else i
	if status == ACTIVE:
		status = CONVERGED if abs(rho - last_rho) < eps else CAP_REACHED
	if status in (FAILED_NAN, FAILED_LAMBDA):
		return np.full(P, np.nan), float(rho), int(iterations), status
	return warp_to_kernel(w, warpmode), float(rho), int(iterations), status


def star_field(R, C, shift=(0.0, 0.0), n_stars=60, sigma=1.2, seed=0, background=100.0):
	"""
	A noise-free field of pixel-integrated Gaussian stars (``simulate._gauss_int``), every star moved by ``shift`` =
	(column, row): the exact image of the reference field at that sub-pixel offset, no interpolation involved.
	"""
	from photometry_amd.simulate import _gauss_int
	rng = np.random.default_rng(seed)
	rows = rng.uniform(8, R - 8, n_stars)
	cols = rng.uniform(8, C - 8, n_stars)
	flux = 10 ** rng.uniform(2.5, 5.0, n_stars)
	img = np.full((R, C), background)
	r = np.arange(R, dtype='float64')
	c = np.arange(C, dtype='float64')
	for k in range(n_stars):
		gr = _gauss_int(r, rows[k] + shift[1], sigma)
		gc = _gauss_int(c, cols[k] + shift[0], sigma)
		img += flux[k] * np.outer(gr, gc)
	return img.astype('float32')
