# -*- coding: utf-8 -*-
"""
The definition of ``tp_motion_interpolate`` / ``tp_motion_star_positions`` (tests/motion_positions_common.py restates it in numpy)
held to the host ``MovementKernel`` without a device: the interpolated kernels bit for bit against scipy's interp1d, the jitter
against ``jitter`` (copies bit for bit, the ECC modes within the derived 1e-10 px), the float32 positions within one float32 step,
and the float32 arithmetic of ``catalog_attime`` (``single``) against ``interpolate`` over float32 positions.
"""
import inspect
import warnings
import numpy as np
import pytest
import motion_positions_common as mp


def test_input_builder():
	for mode in mp.MODES:
		times, kernels = mp.series(mode)
		assert times.shape == (9,) and np.all(np.diff(times) > 0) and kernels.shape == (9, mp.N_PARAMS[mode])
		if mode == 'unchanged':
			continue
		bad = ~np.all(np.isfinite(kernels), axis=1)
		assert list(np.flatnonzero(bad)) == [0, 4]
		tg, kg, first, last = mp.good_of(times, kernels)
		assert len(tg) == 7 and np.all(np.isnan(first)) and np.all(np.isfinite(last))
		q = mp.query_times(times, kernels)
		assert np.isnan(q).sum() == 1 and np.sum(q < tg[0]) >= 3 and np.sum(q > tg[-1]) == 2 and tg[0] in q and tg[-1] in q
		assert all(t in q for t in times)
		t33 = mp.times33(times)
		assert t33.shape == (33,) and np.all(np.diff(t33) > 0) and times[2] in t33 and times[6] in t33
	xy = mp.positions()
	assert xy.shape == (40, 2) and xy.min() >= 0 and xy[:, 0].max() == 2100 and xy[:, 1].max() == 2050


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
def test_interpolation_restatement_is_scipys(mode):
	times, kernels = mp.series(mode)
	mk = mp.loaded(mode, times, kernels)
	q = mp.query_times(times, kernels)
	with warnings.catch_warnings():
		warnings.simplefilter('ignore', RuntimeWarning)
		host = mk._interpolator(q)
		# the host interpolator is deterministic on these inputs, whole array or one time at a time
		np.testing.assert_array_equal(mk._interpolator(q), host)
		np.testing.assert_array_equal(np.stack([mk._interpolator(t) for t in q]), host)
	ref = mp.interpolate_ref(times, kernels, q)
	np.testing.assert_array_equal(ref, host)
	tg = mp.good_of(times, kernels)[0]
	assert np.all(np.isnan(ref[q < tg[0]])) and np.all(np.isfinite(ref[q >= tg[0]])) and np.all(np.isnan(ref[np.isnan(q)]))
	np.testing.assert_array_equal(ref[q > tg[-1]], np.broadcast_to(kernels[-1], (2, kernels.shape[1])))


@pytest.mark.parametrize('mode', mp.MODES)
def test_jitter_and_positions_restatement_against_host(mode):
	times, kernels = mp.series(mode)
	mk = mp.loaded(mode, times, kernels)
	xy, t = mp.positions(), mp.times33(times)
	host = mp.host_jitter(mk, t, xy)
	ref = mp.jitter_ref(mode, mp.matrices_ref(mode, mp.interpolate_ref(times, kernels, t)), xy)
	assert np.array_equal(np.isnan(ref), np.isnan(host))
	if mode in ('unchanged', 'translation'):
		np.testing.assert_array_equal(ref, host)
	else:
		assert np.isnan(host).any() and np.isfinite(host).any()
		err = np.nanmax(np.abs(ref - host))
		print(f"{mode}: restatement - host jitter: max {err:.2e} px")
		assert err <= mp.JITTER_ATOL
		assert np.ptp(host[:, -1, 0]) > 0.1     # every star moves by its own amount
	base = (xy - 100.0).astype('float32')
	for a in range(2):
		with np.errstate(invalid='ignore'):
			exp = (base[:, a][:, None] + host[:, :, a]).astype('float32').astype('float64')
		mp.assert_float32_positions(mp.positions_ref(base[:, a], ref[:, :, a]), exp)


@pytest.mark.parametrize('mode', mp.MODES)
def test_single_restatement_is_catalog_attime(mode):
	"""``single``: what ``catalog_attime`` adds to the float32 catalogue -- ``interpolate`` over float32 positions rounds the
	product to float32 (``np.empty_like(xy)``), subtracts and adds in float32."""
	times, kernels = mp.series(mode)
	mk = mp.loaded(mode, times, kernels)
	xy32 = mp.positions().astype('float32')
	base = (xy32 - np.float32(100.0)).astype('float32')
	t = mp.times33(times)
	with warnings.catch_warnings():
		warnings.simplefilter('ignore', RuntimeWarning)
		host = np.stack([mk.interpolate(tk, xy32) for tk in t], axis=1)
	assert host.dtype == np.float32
	ref = mp.jitter_ref(mode, mp.matrices_ref(mode, mp.interpolate_ref(times, kernels, t)), xy32.astype('float64'), single=True)
	for a in range(2):
		with np.errstate(invalid='ignore'):
			exp = (base[:, a][:, None] + host[:, :, a]).astype('float64')
		assert exp.dtype == np.float64 and (base[:, a][:, None] + host[:, :, a]).dtype == np.float32
		mp.assert_float32_positions(mp.positions_ref(base[:, a], ref[:, :, a], single=True), exp)
	# the float64 definition is NOT this arithmetic: at these coordinates the float32 product is good to 1e-4 px only
	if mode in ('euclidian', 'affine'):
		wide = mp.jitter_ref(mode, mp.matrices_ref(mode, mp.interpolate_ref(times, kernels, t)), xy32.astype('float64'))
		assert np.nanmax(np.abs(wide - ref)) > 1e-6


def test_linpsf_frames_names_no_warpmode_restriction():
	from photometry_amd import pipeline
	src = inspect.getsource(pipeline.linpsf_frames)
	assert 'kernels expected' not in src
	doc = pipeline.linpsf_frames.__doc__
	assert "'euclidian'" in doc and "'affine'" in doc and 'tp_motion_star_positions' in doc


def test_unknown_warpmode_is_refused_on_the_host():
	from photometry_amd.motion import MovementKernel, WARPMODE_CODE
	assert WARPMODE_CODE == {'unchanged': 0, 'translation': 1, 'euclidian': 2, 'affine': 3}
	with pytest.raises(ValueError):
		MovementKernel(warpmode='projective')
	mk = MovementKernel(warpmode='euclidian')
	with pytest.raises(ValueError):
		mk.device_series(ctx=object())     # no series loaded: nothing to put on a device
