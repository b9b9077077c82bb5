# -*- coding: utf-8 -*-
"""
The definition of the LinPSF flux error (``tests/linpsf_err_common.py``) held to itself on the CPU -- closed form,
the one-pass form the kernel uses, scaling, the NaN rule -- and the host side of the feature: the settings switch and the ABI table.
"""
import numpy as np
import pytest
import linpsf_common as lc
import linpsf_err_common as le

T, H, W = 5, 11, 11


@pytest.fixture(scope='module')
def scene():
	_, model = lc.prf_and_model('spoc')
	specs = [lc.design_target(model, 1, 0, T, H, W, seed=1), lc.design_target(model, 3, 1, T, H, W, seed=2)]
	s = le.add_errors(lc.designed_scene(specs, T, H, W, seed=3, nan_fraction=0.02))
	_, so, ti, pr, pc = lc.fit_inputs(s)
	return s, (so, ti, pr, pc)


def test_one_star_constant_sigma_is_the_closed_form(scene):
	s, fit = scene
	so, ti, pr, pc = fit
	psf = le.oracle_psf('spoc', s.stamps[0])
	sigma = 7.25
	err = np.where(np.isfinite(s.images[0]), np.float32(sigma), np.float32(np.nan)).astype('float32')
	got = le.flux_err_series(psf, s.images[0], err, pr[so[0]:so[1]], pc[so[0]:so[1]], int(ti[0]))
	for k in range(T):
		A, _ = le.design_matrix(psf, s.images[0][:, :, k], pr[so[0]:so[1], k], pc[so[0]:so[1], k])
		np.testing.assert_allclose(got[k], sigma / np.sqrt(np.sum(A[:, 0]**2)), rtol=1e-12)


def test_row_form_equals_the_one_pass_form(scene):
	s, fit = scene
	so, ti, pr, pc = fit
	for i in range(2):
		psf = le.oracle_psf('spoc', s.stamps[i])
		a, b = so[i], so[i + 1]
		row = le.flux_err_series(psf, s.images[i], s.images_err[i], pr[a:b], pc[a:b], int(ti[i]), form='row')
		pwp = le.flux_err_series(psf, s.images[i], s.images_err[i], pr[a:b], pc[a:b], int(ti[i]), form='pWp')
		assert np.all(np.isfinite(row)) and np.all(row > 0)
		np.testing.assert_allclose(pwp, row, rtol=1e-12)


def test_doubling_the_errors_doubles_the_result_exactly(scene):
	s, fit = scene
	ref = le.restate_target(s, fit, 1)
	twice = le.restate_target(s, fit, 1, images_err=(s.images_err * np.float32(2)))
	np.testing.assert_array_equal(twice, 2.0 * ref)


def test_nan_rule(scene):
	s, fit = scene
	# target 0 has one star, in the middle of the stamp: a corner pixel is outside its cut-off disc (m_px = 0) -- NaN all the same
	ref0 = le.restate_target(s, fit, 0)
	err = s.images_err.copy()
	good = np.argwhere(np.isfinite(s.images[0][:, :, 2]))
	corner = [g for g in good if tuple(g) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))][0]
	err[0, corner[0], corner[1], 2] = np.nan
	got = le.restate_target(s, fit, 0, images_err=err)
	assert np.isnan(got[2])
	np.testing.assert_array_equal(np.delete(got, 2), np.delete(ref0, 2))
	ref = le.restate_target(s, fit, 1)
	bad = np.argwhere(~np.isfinite(s.images[1]))
	assert len(bad) > 0
	# NaN (or anything) in err where the image is not finite changes nothing
	err = s.images_err.copy()
	for (i, j, k) in bad:
		err[1, i, j, k] = np.float32(np.inf) if (i + j) % 2 else np.float32(-5.0)
	np.testing.assert_array_equal(le.restate_target(s, fit, 1, images_err=err), ref)
	# a cadence without a good pixel gives 0
	img = s.images.copy()
	img[1, :, :, 3] = np.nan
	assert le.restate_target(s, fit, 1, images=img)[3] == 0.0


def test_settings_switch(tmp_path, monkeypatch):
	from photometry_amd import plugins
	monkeypatch.delenv('TESSPHOT_SETTINGS', raising=False)
	assert plugins.load_settings().getboolean('linpsf', 'flux_errors') is False
	assert plugins.LinPSFPhotometry.flux_errors() is False
	f = tmp_path / 'settings.ini'
	f.write_text('[linpsf]\nflux_errors = true\n')
	assert plugins.load_settings(str(f)).getboolean('linpsf', 'flux_errors') is True
	monkeypatch.setenv('TESSPHOT_SETTINGS', str(f))
	assert plugins.LinPSFPhotometry.flux_errors() is True
	# the other defaults are still there beside it
	assert plugins.load_settings().getboolean('halo', 'enabled') is False


def test_abi_table_has_the_entries():
	import os
	import re
	import conftest
	from photometry_amd import _lib
	src = open(os.path.join(conftest.ROOT, 'include', 'tessphot_hip.h')).read()
	src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
	for name, arity in (('tp_linpsf_flux_err', 17), ('tp_linpsf_flux_err_xy', 18)):
		assert name in _lib.SIGNATURES
		m = re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
		assert m, name
		n = len([p for p in m.group(1).split(',') if p.strip()])
		assert n == arity == len(_lib.SIGNATURES[name][1])
