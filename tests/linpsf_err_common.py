# -*- coding: utf-8 -*-
"""
The CPU restatement of the LinPSF flux error (``tp_linpsf_flux_err``, include/tessphot_hip.h) and the helpers the
host test (``test_linpsf_err_host.py``) and the device tests (``test_gpu_linpsf_err.py``, ``test_gpu_linpsf_err_plugin.py``) share.

The reference has no definition (linpsf_photometry.py:169 writes NaN), so it is written down here, per cadence, in numpy float64:
``good`` = finite image pixels; ``A`` = the design matrix of the fit, built with ``oracle.psf.PSF.integrate_to_image`` exactly as
``oracle/linpsf.py:68-71``; ``m`` = row ``t`` of ``pinv(A^T A) A^T`` (``np.linalg.pinv``, rcond 1e-15), written out explicitly;
``flux_err = sqrt(sum_good (m_px * err_px)^2)`` as a plain sum: a non-finite ``err`` at a good pixel gives NaN, no good pixel gives 0.
"""

import numpy as np


def design_matrix(psf, img, rows, cols, cutoff_radius=5):
	"""``A`` and ``good_pixels`` of one cadence (oracle/linpsf.py:65-71): ``img`` ``(H, W)``, ``rows`` / ``cols`` ``(S,)``."""
	good_pixels = np.isfinite(img)
	npx = int(np.sum(good_pixels))
	nstars = len(rows)
	A = np.empty([npx, nstars], dtype='float64')
	for col in range(nstars):
		params0 = np.atleast_2d([rows[col], cols[col], 1.])
		A[:, col] = psf.integrate_to_image(params0, cutoff_radius=cutoff_radius)[good_pixels].flatten()
	return A, good_pixels


def cadence_flux_err(A, err, staridx, form='row'):
	"""The definition for one cadence: ``A`` ``(npx, S)``, ``err`` ``(npx,)`` float64 (the float32 values widened).
	``form='row'``: the explicit row of ``pinv(A^T A) A^T``; ``form='pWp'``: ``W = A^T diag(err^2) A``, ``var = p^T W p``."""
	if A.shape[0] == 0:
		return 0.0
	if not np.all(np.isfinite(err)):
		return np.nan
	p = np.linalg.pinv(A.T @ A)[staridx, :]
	if form == 'row':
		m = A @ p
		return float(np.sqrt(np.sum((m * err)**2)))
	W = A.T @ (A * (err**2)[:, None])
	return float(np.sqrt(max(p @ W @ p, 0.0)))


def flux_err_series(psf, images, images_err, pos_rows, pos_cols, staridx, cutoff_radius=5, form='row'):
	"""``flux_err`` ``(T,)`` of one target: ``images`` / ``images_err`` ``(H, W, T)`` float32, ``pos_rows`` / ``pos_cols`` ``(S, T)`` the
	positions of the fitted stars, ``staridx`` the target's index among them."""
	T = images.shape[2]
	out = np.empty(T)
	for k in range(T):
		A, good = design_matrix(psf, images[:, :, k], pos_rows[:, k], pos_cols[:, k], cutoff_radius)
		out[k] = cadence_flux_err(A, images_err[:, :, k][good].astype('float64'), staridx, form)
	return out


def add_errors(scene, readnoise=10.0):
	"""An error cube for a ``linpsf_common.designed_scene``: ``sqrt(|image| + readnoise^2)`` as float32 (NaN where the image is)."""
	with np.errstate(invalid='ignore'):
		scene.images_err = np.sqrt(np.abs(scene.images.astype('float64')) + readnoise**2).astype('float32')
	return scene


def oracle_psf(kind, stamp):
	"""The oracle's PSF of a stamp on the PRF samples ``kind`` of ``linpsf_common.prf_and_model``."""
	from oracle import psf as opsf
	import linpsf_common as lc
	prf, _ = lc.prf_and_model(kind)
	return opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(stamp))


def restate_target(scene, fit, i, kind='spoc', cutoff_radius=5, images=None, images_err=None):
	"""The restatement for target ``i`` of a designed scene; ``fit`` = ``(star_offsets, target_index, pos_row, pos_col)``."""
	so, ti, pr, pc = fit
	a, b = int(so[i]), int(so[i + 1])
	images = scene.images if images is None else images
	images_err = scene.images_err if images_err is None else images_err
	return flux_err_series(oracle_psf(kind, scene.stamps[i]), images[i], images_err[i], pr[a:b], pc[a:b], int(ti[i]), cutoff_radius)


def assert_flux_err(got, ref, rtol=1e-8, label=''):
	"""The device's series against the restatement: NaN pattern equal, finite values to ``rtol`` relative."""
	got, ref = np.asarray(got), np.asarray(ref)
	np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=label + ' NaN pattern')
	ok = ~np.isnan(ref)
	np.testing.assert_allclose(got[ok], ref[ok], rtol=rtol, atol=0.0, err_msg=label)
