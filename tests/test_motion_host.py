# -*- coding: utf-8 -*-
"""
CPU checks of the image-motion feature: the behaviours of the reference's tests/test_imagemotion.py on MovementKernel (with the
CPU restatement tests/motion_common.py where a kernel has to be computed), the Scharr filter pinned by hand, and the known-answer
recovery of sub-pixel shifts by the restatement.
"""
import json
import numpy as np
import pytest
from photometry_amd.motion import MovementKernel, movement_from_header
import motion_common as mc

# measured with the restatement on noise-free 256 x 256 fields of pixel-integrated Gaussian stars, |shift| <= 0.5 px
# (DESIGN.md section 9): worst errors 0.0070 (translation), 0.0070 (euclidian), 0.0105 (affine) px
KNOWN_ANSWER_TOL = {'translation': 0.01, 'euclidian': 0.01, 'affine': 0.015}


def test_invalid_warpmode():
	with pytest.raises(ValueError) as e:
		MovementKernel(warpmode='not-a-warpmode')
	assert str(e.value) == "Invalid warpmode"


def test_unchanged_gives_empty_kernel():
	mk = MovementKernel(warpmode='unchanged', image_ref=np.ones((10, 10)))
	assert mk.calc_kernel(np.ones((10, 10))) == []
	np.testing.assert_array_equal(mk.apply_kernel([[1.0, 2.0], [3.0, 4.0]], []), 0)


def test_no_reference_image():
	with pytest.raises(RuntimeError) as e:
		MovementKernel(warpmode='translation').calc_kernel(np.ones((10, 10)))
	assert str(e.value) == "Reference image not defined"


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
def test_interpolate_before_load_series(mode):
	with pytest.raises(ValueError) as e:
		MovementKernel(warpmode=mode).interpolate(1.0, [[1.0, 2.0]])
	assert str(e.value) == "Interpolator is not defined. "


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
def test_wrong_kernel_shape(mode):
	mk = MovementKernel(warpmode=mode)
	with pytest.raises(ValueError) as e:
		mk.load_series(np.arange(4.0), np.zeros((4, mk.n_params + 1)))
	assert str(e.value).startswith(f"Wrong shape of kernels. Anticipated (4,{mk.n_params})")


def test_wcs_is_not_available():
	mk = MovementKernel(warpmode='wcs')
	assert mk.n_params == 1
	for call in (lambda: mk.apply_kernel([[1.0, 2.0]], None), lambda: mk.load_series([1.0], ['']), lambda: mk.interpolate(1.0, [[1.0, 2.0]])):
		with pytest.raises(NotImplementedError, match='astropy.wcs'):
			call()
	with pytest.raises(NotImplementedError, match='astropy.wcs'):
		MovementKernel(warpmode='translation', wcs_ref='header')


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
def test_same_image_gives_no_movement(mode):
	"""test_imagemotion.py: the reference image against itself -> every delta_pos within 1e-5 (kernel from the restatement)."""
	img = mc.star_field(96, 96, seed=4)
	prep = mc.prepare_flux(img)
	kernel, rho, iters, status = mc.ecc(prep, prep, mode)
	assert status == mc.CONVERGED
	mk = MovementKernel(warpmode=mode)
	xy = np.array([[0.0, 0.0], [50.5, 20.25], [95.0, 95.0], [1000.0, 2000.0]])
	np.testing.assert_allclose(mk.apply_kernel(xy, kernel), 0, atol=1e-5)


def test_scharr_constant_and_ramp():
	np.testing.assert_array_equal(mc.scharr(np.full((9, 11), 0.37, dtype='float32')), 0)
	a = 0.01
	ramp = (a * np.arange(12, dtype='float64'))[None, :].repeat(10, axis=0).astype('float32')
	s = mc.scharr(ramp)
	# interior: h = 0, v = 2a (the [1, 0, -1] difference across two pixels), magnitude sqrt(4a^2 / 2) = sqrt(2) a
	np.testing.assert_allclose(s[1:-1, 1:-1], np.sqrt(2) * a, rtol=1e-5)
	# the 'reflect' border repeats the edge pixel: the difference at the first column spans one pixel only
	np.testing.assert_allclose(s[:, 0], a / np.sqrt(2), rtol=1e-5)
	np.testing.assert_allclose(s[:, -1], a / np.sqrt(2), rtol=1e-5)
	assert s.dtype == np.float32


def test_prepare_flux_nan_spreads_then_zero():
	img = mc.star_field(32, 32, seed=2) + np.random.default_rng(2).normal(0, 5, (32, 32)).astype('float32')
	img[10, 15] = np.nan
	p = mc.prepare_flux(img)
	assert p.dtype == np.float32 and np.all(np.isfinite(p))
	# the NaN reaches its 3 x 3 neighbourhood through the filter and no further, then becomes 0
	np.testing.assert_array_equal(p[9:12, 14:17], 0)
	assert np.count_nonzero(p == 0) == 9
	# flat and all-NaN frames: nothing but zeros
	np.testing.assert_array_equal(mc.prepare_flux(np.full((8, 8), 5.0)), 0)
	np.testing.assert_array_equal(mc.prepare_flux(np.full((8, 8), np.nan)), 0)


def test_prepare_flux_range():
	"""log10 of the min-shifted flux rescaled to [-1, 1]: both transforms are monotonic, the extremes land on -1 and 1."""
	img = mc.star_field(24, 24, seed=3).astype('float64')
	f = np.log10(img - img.min() + 1)
	f1 = -1 + 2 * (f - f.min()) / (f.max() - f.min())
	np.testing.assert_allclose(mc.prepare_flux(img), mc.scharr(f1.astype('float32')), atol=2e-6)


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
def test_known_answer_recovery(mode):
	R = C = 128
	ref = mc.star_field(R, C, seed=11, n_stars=30)
	tmpl = mc.prepare_flux(ref)
	rng = np.random.default_rng(7)
	for _ in range(3):
		s = rng.uniform(-0.5, 0.5, 2)
		kernel, rho, iters, status = mc.ecc(tmpl, mc.prepare_flux(mc.star_field(R, C, shift=s, seed=11, n_stars=30)), mode)
		assert status == mc.CONVERGED and 1 <= iters < 50
		shift = kernel[[2, 5]] if mode == 'affine' else kernel[:2]
		assert np.abs(shift - s).max() < KNOWN_ANSWER_TOL[mode], (mode, shift, s)


def test_movement_from_header_json_round_trip(tmp_path):
	from photometry_amd import frameio
	rng = np.random.default_rng(1)
	T = 6
	kernels = rng.normal(0, 0.3, (T, 2))
	kernels[2] = np.nan
	time = 1500.0 + np.arange(T) / 48.0 + rng.uniform(0, 1e-3, T)
	path = frameio.write_stack(str(tmp_path / 'x.tpstack'), {'images': np.zeros((T, 4, 5), dtype='float32')}, time=time,
		movement_kernel=kernels, movement_warpmode='translation', movement_ref_frame=3)
	hdr = frameio.read_header(path)
	back = np.asarray(hdr['attrs']['movement_kernel']['kernels'], dtype='float64')
	np.testing.assert_array_equal(back, kernels)               # JSON floats round-trip exactly (NaN included)
	assert hdr['attrs']['movement_kernel']['warpmode'] == 'translation' and hdr['attrs']['movement_kernel']['ref_frame'] == 3
	mk = movement_from_header(hdr)
	ref = MovementKernel(warpmode='translation')
	ref.load_series(time, kernels)
	np.testing.assert_array_equal(mk.jitter(time, 10.0, 20.0), ref.jitter(time, 10.0, 20.0))
	assert movement_from_header(frameio.read_header(frameio.write_stack(str(tmp_path / 'y.tpstack'),
		{'images': np.zeros((T, 4, 5), dtype='float32')}))) is None
	json.dumps(hdr['attrs'])
