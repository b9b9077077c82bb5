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


# ---- the inputs of the off-grid device tests (tests/test_gpu_motion.py), held honest on the restatement -----------

def _parent_star_field(R, C, shift=(0.0, 0.0), n_stars=60, sigma=1.2, seed=0, background=100.0):
	"""star_field as it was before it learnt ``warp`` and ``margin``, kept here to pin the images of the existing callers."""
	from photometry_amd.simulate import _gauss_int
	rng = np.random.default_rng(seed)
	rows = rng.uniform(8, R - 8, n_stars)
	cols = rng.uniform(8, C - 8, n_stars)
	flux = 10 ** rng.uniform(2.5, 5.0, n_stars)
	img = np.full((R, C), background)
	r = np.arange(R, dtype='float64')
	c = np.arange(C, dtype='float64')
	for k in range(n_stars):
		img += flux[k] * np.outer(_gauss_int(r, rows[k] + shift[1], sigma), _gauss_int(c, cols[k] + shift[0], sigma))
	return img.astype('float32')


def test_star_field_without_warp_is_unchanged():
	for R, C, kw in [(96, 96, {'seed': 4}), (128, 128, {'seed': 11, 'n_stars': 30, 'shift': (0.21, -0.37)}), (384, 320, {'seed': 11, 'n_stars': 61,
		'shift': (-0.31, 0.42)}), (32, 32, {'seed': 2})]:
		np.testing.assert_array_equal(mc.star_field(R, C, **kw), _parent_star_field(R, C, **kw))
	# a pure shift written as a warp is the same field to the rounding of the star centres
	a = mc.star_field(64, 80, shift=(0.3, -0.2), seed=5, n_stars=10)
	b = mc.star_field(64, 80, warp=mc.shift_warp(0.3, -0.2), seed=5, n_stars=10)
	np.testing.assert_allclose(a, b, rtol=1e-6)
	# the warp moves the centre of a star to warp @ [column, row, 1]: the flux-weighted centroid of one star follows it
	W = mc.rot_warp(0.04, 1.5, -2.0)
	one = mc.star_field(90, 120, n_stars=1, seed=8, warp=W, margin=30, background=0.0).astype('float64')
	ref = mc.star_field(90, 120, n_stars=1, seed=8, margin=30, background=0.0).astype('float64')
	yy, xx = np.mgrid[0:90, 0:120]
	p = np.array([(ref * xx).sum(), (ref * yy).sum()]) / ref.sum()
	q = np.array([(one * xx).sum(), (one * yy).sum()]) / one.sum()
	np.testing.assert_allclose(q, W @ [p[0], p[1], 1.0], atol=1e-4)


def test_ecc_history_and_step():
	a, b = (mc.prepare_flux(mc.case_field(33, 130, warp=w)) for w in (None, mc.SMALL_SHIFTS[0]))
	plain = mc.ecc(a, b, 'euclidian')
	full = mc.ecc(a, b, 'euclidian', history=True)
	assert len(plain) == 4 and len(full) == 5
	for u, v in zip(plain, full[:4]):
		np.testing.assert_array_equal(u, v)
	hist = full[4]
	assert len(hist) == full[2] and hist[-1]['rho'] == full[1]
	np.testing.assert_array_equal(mc.warp_to_kernel(hist[-1]['warp'], 'euclidian'), full[0])
	assert all(h['N'] == 33 * 130 and 1 <= h['cond'] < 1e8 for h in hist)
	# the history of a capped run is the head of the full one: a cap only cuts the series
	for n in (1, 3):
		kern, rho, it, status, h = mc.ecc(a, b, 'euclidian', max_iter=n, history=True)
		assert (it, status) == (n, mc.CAP_REACHED) and rho == hist[n - 1]['rho']
		np.testing.assert_array_equal(h[-1]['warp'], hist[n - 1]['warp'])
	step = mc.ecc_step(a, b, 'euclidian')
	for u, v in zip(step, mc.ecc(a, b, 'euclidian', max_iter=1)):
		np.testing.assert_array_equal(u, v)
	assert step[2] == 1 and step[3] == mc.CAP_REACHED


def test_ragged_stack_inputs():
	for R, C in mc.RAGGED_SHAPES:
		st = mc.ragged_stack(R, C)
		assert st.shape == (4, R, C) and st.dtype == np.float32
		assert np.all(np.isfinite(st[0])) and np.all(np.isnan(st[2])) and np.all(st[3] == st[3, 0, 0])
		pos = mc.nan_positions(R, C)
		assert {(0, 0), (0, C - 1), (R - 1, 0), (R - 1, C - 1)} <= set(pos)
		assert all(0 <= r < R and 0 <= c < C for r, c in pos)
		assert np.count_nonzero(np.isnan(st[1])) == len(set(pos))
		# neither a whole prepare tile (16 x 64) nor a whole iteration tile (32 x 128) both ways, but for the one on-grid control
		assert (R, C) == (16, 64) or R % 16 or C % 64
		p = mc.prepare_flux(st[0])
		assert np.all(np.isfinite(p)) and np.count_nonzero(p) > 0


@pytest.mark.parametrize('shape', mc.ONE_STEP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_step_inputs(shape):
	"""One step is a fair comparison (conditioning), and the warps that are to leave the frame do leave it after MASK_STEPS steps."""
	R, C = shape
	names, flags, prep = mc.one_step_prepared(R, C)
	assert sum(flags) >= 1
	for mode in mc.MODES:
		for k, name in enumerate(names):
			kern, rho, it, status, hist = mc.ecc_step(prep[0], prep[k], mode, history=True)
			assert it == 1 and hist[0]['N'] == R * C and hist[0]['cond'] <= mc.TINY_MAX_COND, (mode, name)
			assert status in (mc.CAP_REACHED, mc.FAILED_LAMBDA), (mode, name, status)
			if flags[k]:
				kern, rho, it, status, hist = mc.ecc(prep[0], prep[k], mode, max_iter=mc.MASK_STEPS, eps=0.0, history=True)
				assert (it, status) == (mc.MASK_STEPS, mc.CAP_REACHED), (mode, name, it, status)
				assert hist[-1]['N'] <= mc.MASK_SHARE * R * C, (mode, name, hist[-1]['N'] / (R * C))
				assert all(h['cond'] <= mc.TINY_MAX_COND and h['N'] >= 0.5 * R * C for h in hist), (mode, name)


@pytest.mark.parametrize('shape,mode', mc.TINY_CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_tiny_inputs_are_conditioned(shape, mode):
	prep = mc.tiny_prepared(*shape)
	kern, rho, it, status, hist = mc.ecc_step(prep[0], prep[1], mode, history=True)
	assert (it, status) == (1, mc.CAP_REACHED) and np.all(np.isfinite(kern)) and 0.9 < rho < 1
	assert hist[0]['cond'] <= mc.TINY_MAX_COND and hist[0]['N'] >= 2 * mc.N_PARAMS[mode], (hist[0]['cond'], hist[0]['N'])


def test_tiny_cases_cover_what_can_be_covered():
	for s in [(3, 3), (5, 4), (7, 7)]:
		assert (s, 'translation') in mc.TINY_CASES
	assert {s for s, _ in mc.TINY_CASES} == set(mc.TINY_SHAPES)
	assert sorted(mc.TINY_CASES + mc.TINY_SINGULAR) == sorted((s, m) for s in mc.TINY_SHAPES for m in mc.MODES)
	# what is left out is out of the condition, not merely inconvenient
	for shape, mode in mc.TINY_SINGULAR:
		prep = mc.tiny_prepared(*shape)
		hist = mc.ecc_step(prep[0], prep[1], mode, history=True)[4]
		assert hist[0]['cond'] > mc.TINY_MAX_COND


@pytest.mark.parametrize('mode', mc.MODES)
@pytest.mark.parametrize('shape', mc.CONVERGED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_converged_inputs(shape, mode):
	"""Every converged case converges in the restatement, with the iteration-count margin, and meets its known answer where one is claimed."""
	names, warps, known, frames = mc.converged_stack(shape, mode)
	prep = [mc.prepare_flux(f) for f in frames]
	for k, name in enumerate(names):
		kern, rho, it, status, hist = mc.ecc(prep[0], prep[k], mode, history=True)
		assert status == mc.CONVERGED and it < 50, (name, status, it)
		assert mc.margin_ok(hist, 1e-6), (name, mc.loop_test_values(hist, 1e-6))
		if known[k]:
			assert np.abs(kern - mc.warp_to_kernel(warps[k], mode)).max() < KNOWN_ANSWER_TOL[mode], (name, kern)
		if name in ('l0', 'l1', 'r04'):
			assert hist[-1]['N'] <= mc.MASK_SHARE * shape[0] * shape[1], (name, hist[-1]['N'])
	if mode == 'translation':
		assert sum(known) >= 4
	if mode == 'euclidian':
		assert all(known) == (shape == (200, 333))


def test_ref_middle_inputs():
	frames = mc.ref_middle_stack()
	ref = mc.REF_MIDDLE['ref_frame']
	assert 0 < ref < len(frames) - 1
	prep = [mc.prepare_flux(f) for f in frames]
	for k in range(len(frames)):
		kern, rho, it, status, hist = mc.ecc(prep[ref], prep[k], mc.REF_MIDDLE['mode'], history=True)
		assert status == mc.CONVERGED and mc.margin_ok(hist, 1e-6), (k, status)
		true = np.subtract(mc.REF_MIDDLE['shifts'][k], mc.REF_MIDDLE['shifts'][ref])
		assert np.abs(kern - true).max() < KNOWN_ANSWER_TOL['translation']


@pytest.mark.parametrize('mode', mc.MODES)
def test_cap_inputs(mode):
	"""eps = 0: no frame of the cap stack fails, so every one must end CAP_REACHED at the cap; the mixed chunk holds a frame of each kind."""
	assert mc.CAPS == (0, 1, 3, 5, 13, 37)     # inside no poll, the first (4), the second (12), the third (28) and the fourth (60) interval
	prep = [mc.prepare_flux(f) for f in mc.cap_stack()]
	assert len(prep) == 9
	for k in range(len(prep)):
		kern, rho, it, status, hist = mc.ecc(prep[0], prep[k], mode, max_iter=max(mc.CAPS), eps=0.0, history=True)
		assert (it, status) == (max(mc.CAPS), mc.CAP_REACHED) and np.all(np.isfinite(kern)), (k, it, status)
		assert all(np.isfinite(h['rho']) and h['cond'] <= mc.TINY_MAX_COND for h in hist)
	kern, rho, it, status = mc.ecc(prep[0], prep[1], mode, max_iter=0, eps=0.0)
	assert (rho, it, status) == (-1.0, 0, mc.CAP_REACHED)
	np.testing.assert_array_equal(kern, mc.warp_to_kernel(np.eye(2, 3), mode))
	prep = [mc.prepare_flux(f) for f in mc.mixed_stack()]
	res = [mc.ecc(prep[0], p, mode, max_iter=mc.MIXED_CAP, history=True) for p in prep]
	status = [r[3] for r in res]
	assert status[:3] == [mc.CONVERGED, mc.CONVERGED, mc.CAP_REACHED] and status[3] >= mc.FAILED_NAN and status[4] >= mc.FAILED_NAN, status
	assert res[0][2] < res[1][2] < mc.MIXED_CAP == res[2][2] and 4 < res[1][2]     # stops in the first poll, in the second, and at the cap
	assert all(mc.margin_ok(r[4], 1e-6) for r in res[:3])
