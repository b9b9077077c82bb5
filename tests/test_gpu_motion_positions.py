# -*- coding: utf-8 -*-
"""
A loaded series of movement kernels applied to many positions on the device (``tp_motion_interpolate`` /
``tp_motion_star_positions``, csrc/motion.hip) against the host ``MovementKernel`` and the numpy restatement
tests/motion_positions_common.py: the interpolated kernels bit for bit, the jitter of every warp mode, the float32 positions the
LinPSF fit reads, batch independence, ``linpsf_frames`` under euclidian and affine kernels against the LinPSF plugin,
``tessphot_frames(movement=)`` against the plugin's ``pos_corr``, and the refusals.
"""
import warnings
from types import SimpleNamespace
import numpy as np
import pytest
import motion_positions_common as mp

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.fixture(scope='module')
def host_jitters():
	"""mode -> (times, kernels, t, xy, the host jitter (40, 33, 2)): computed once, shared, never written to."""
	out = {}
	for mode in mp.MODES:
		times, kernels = mp.series(mode)
		t, xy = mp.times33(times), mp.positions()
		j = mp.host_jitter(mp.loaded(mode, times, kernels), t, xy)
		j.setflags(write=False)
		out[mode] = (times, kernels, t, xy, j)
	return out


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
def test_interpolation_bit_for_bit(ctx, mode):
	times, kernels = mp.series(mode)
	mk = mp.loaded(mode, times, kernels, ctx=ctx)
	q = mp.query_times(times, kernels)
	with warnings.catch_warnings():
		warnings.simplefilter('ignore', RuntimeWarning)
		host = mk._interpolator(q)
		np.testing.assert_array_equal(mk._interpolator(q), host)     # the host interpolator is deterministic on these inputs
	got = mk.interpolate_many(q)
	assert got.shape == host.shape and np.isnan(host).any() and np.isfinite(host).any()
	np.testing.assert_array_equal(got, host)
	np.testing.assert_array_equal(got, mp.interpolate_ref(times, kernels, q))


@pytest.mark.parametrize('mode', mp.MODES)
def test_jitter_many_against_host_jitter(ctx, host_jitters, mode):
	times, kernels, t, xy, host = host_jitters[mode]
	mk = mp.loaded(mode, times, kernels, ctx=ctx)
	got = mk.jitter_many(t, xy[:, 0], xy[:, 1]).to_host()
	assert got.shape == (40, 33, 2) and got.dtype == np.float64
	assert np.array_equal(np.isnan(got), np.isnan(host))
	if mode in ('unchanged', 'translation'):
		np.testing.assert_array_equal(got, host)
	else:
		err = np.nanmax(np.abs(got - host))
		print(f"{mode}: device - host jitter: max {err:.2e} px")
		assert err <= mp.JITTER_ATOL
	# the series stays on the device: a second call uploads nothing
	loaded = mk._d_loaded
	mk.jitter_many(t[:3], xy[:2, 0], xy[:2, 1])
	assert mk._d_loaded is loaded


def _selected_positions(ctx, mk, t, xy, base, out_index, n_out, pitch, single=False):
	"""tp_motion_star_positions into sentinel-filled (n_out, pitch) arrays; the host copies."""
	fill = np.full((n_out, pitch), SENTINEL)
	pos = (ctx.array(fill), ctx.array(fill))
	pc, pr, _ = mk.star_positions(t, xy, base[:, 0], base[:, 1], out_index, n_out, pitch=pitch, single=single, pos=pos)
	return pc.to_host(), pr.to_host()


@pytest.mark.parametrize('mode', mp.MODES)
def test_float32_positions(ctx, host_jitters, mode):
	times, kernels, t, xy, host = host_jitters[mode]
	mk = mp.loaded(mode, times, kernels, ctx=ctx)
	n, T, pitch = len(xy), len(t), len(t) + 7
	base = (xy - 100.0).astype('float32')
	keep = np.random.default_rng(8).random(n) >= 0.3
	assert 0.2 < np.mean(~keep) < 0.4
	out_index = np.full(n, -1, dtype='int64')
	order = np.random.default_rng(9).permutation(int(keep.sum()))    # the selection need not keep the order
	out_index[keep] = order
	n_out = len(order)
	got = _selected_positions(ctx, mk, t, xy, base, out_index, n_out, pitch)
	for a in range(2):
		assert np.all(got[a][:, T:] == SENTINEL)
		with np.errstate(invalid='ignore'):
			exp = (base[keep, a][:, None] + host[keep, :, a]).astype('float32').astype('float64')
		mp.assert_float32_positions(got[a][order, :T], exp)
	# unselected stars are not written: a selection of the first half leaves the rows of the second half alone
	half = np.where(np.arange(n) < n // 2, np.arange(n), -1)
	part = _selected_positions(ctx, mk, t, xy, base, half, n, pitch)
	for a in range(2):
		assert np.all(part[a][n // 2:] == SENTINEL) and np.all(part[a][:n // 2, T:] == SENTINEL)
		assert not np.any(part[a][:n // 2, :T] == SENTINEL)


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
def test_batch_independence_and_reproducibility(ctx, host_jitters, mode):
	times, kernels, t, xy, _ = host_jitters[mode]
	mk = mp.loaded(mode, times, kernels, ctx=ctx)
	n, T = len(xy), len(t)
	base = (xy - 100.0).astype('float32')
	index = np.arange(n)
	for single in (False, True):
		def run(sel):
			pc, pr, j = mk.star_positions(t, xy[sel], base[sel, 0], base[sel, 1], np.arange(len(sel)), len(sel), single=single, want_jitter=True)
			return pc.to_host().tobytes(), pr.to_host().tobytes(), j.to_host().tobytes()
		whole = run(index)
		assert run(index) == whole     # two identical calls give identical bytes
		for i in (0, 17, n - 1):
			alone = run(index[i:i + 1])
			for a, w in zip(alone[:2], whole[:2]):
				assert a == w[i * T * 8:(i + 1) * T * 8]
			assert alone[2] == whole[2][i * T * 16:(i + 1) * T * 16]


def _rotating_series(mode, time, centre=(302.0, 167.0)):
	"""Kernels that turn the field about ``centre`` (column, row) by up to 5e-3 rad, one of them NaN."""
	T = len(time)
	theta = 5e-3 * np.sin(np.arange(T) * 1.3 + 0.4)
	c, s = np.cos(theta), np.sin(theta)
	dx = centre[0] - (c * centre[0] - s * centre[1]) + 0.02 * np.cos(np.arange(T))
	dy = centre[1] - (s * centre[0] + c * centre[1]) - 0.03 * np.sin(np.arange(T))
	if mode == 'euclidian':
		k = np.column_stack((dx, dy, theta))
	else:
		k = np.column_stack((c * 1.0002, -s, dx, s + 1e-4, c * 0.9999, dy))
	k[4] = np.nan
	return k


@pytest.mark.parametrize('mode', ['euclidian', 'affine'])
def test_linpsf_frames_equals_plugin(ctx, tmp_path, mode):
	from photometry_amd import pipeline, STATUS
	from photometry_amd import psf as hpsf, simulate
	from photometry_amd.plugins import LinPSFPhotometry
	from photometry_amd.source import MemoryStampSource
	from test_gpu_psf_frames import _region
	T = 10
	frames, row0, col0, time, quality, cat, targets, _ = _region(T=T)
	prf = simulate.synthetic_prf(seed=3)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	stack = pipeline.FrameStack(ctx, {k: np.moveaxis(v, 2, 0) for k, v in frames.items()}, row0, col0)
	timecorr = np.full(T, 1e-4)
	tref = time - timecorr
	mk = mp.loaded(mode, tref, _rotating_series(mode, time), ctx=ctx)
	assert len(mk._series_good[0]) == T - 1
	batch = pipeline.linpsf_frames(ctx, stack, targets, cat, time, quality, model, movement=mk, timecorr=timecorr)
	src = MemoryStampSource(frames, row0, col0, time, timecorr, np.arange(T), quality, cat, targets=targets, prf=model, movement=mk)
	n_loose = 0
	first_last = []
	for i in range(len(targets['starid'])):
		b = batch[i]
		with LinPSFPhotometry(int(targets['starid'][i]), src, str(tmp_path), ctx=ctx) as pho:
			status = pho.do_photometry()
			assert tuple(pho.stamp) == b['stamp']
			assert status.value == b['status'], (i, status, b['status'])
			assert status != STATUS.ERROR
			# the plugin's positions of the stamp's whole catalogue at every cadence, and the device's of the same catalogue
			c0 = pho.catalog
			with warnings.catch_warnings():
				warnings.simplefilter('ignore', RuntimeWarning)
				at = [pho.catalog_attime(tk) for tk in tref]
			plug_c = np.stack([np.asarray(a['column_stamp'], dtype='float64') for a in at], axis=1)
			plug_r = np.stack([np.asarray(a['row_stamp'], dtype='float64') for a in at], axis=1)
			m = len(c0['column'])
			pc, pr, _ = mk.star_positions(tref, np.column_stack((c0['column'], c0['row'])), c0['column_stamp'], c0['row_stamp'], np.arange(m), m, single=True)
			pc, pr = pc.to_host(), pr.to_host()
			first_last.append(np.column_stack((pc[:, 1], pc[:, 3])))
			if np.array_equal(pc, plug_c, equal_nan=True) and np.array_equal(pr, plug_r, equal_nan=True):
				np.testing.assert_array_equal(pho.lightcurve['flux'], b['flux'])
				np.testing.assert_array_equal(pho.lightcurve['flux_err'], b['flux_err'])
			else:
				n_loose += 1
				print(f"target {i}: {np.sum(pc != plug_c) + np.sum(pr != plug_r)} of {2 * pc.size} positions differ from the plugin's")
				np.testing.assert_allclose(pho.lightcurve['flux'], b['flux'], rtol=1e-5)
				np.testing.assert_allclose(pho.lightcurve['flux_err'], b['flux_err'], rtol=1e-5)
			assert np.isfinite(b['flux']).sum() >= T - 1
	assert n_loose <= 1
	# the field rotates: stars at opposite ends of the region move differently between two cadences
	fl = np.concatenate(first_last)
	spread = np.ptp(fl[:, 1] - fl[:, 0])
	print(f"{mode}: spread of the column movement over the region: {spread:.3f} px")
	assert spread > 0.1


def _aperture_region():
	from test_gpu_psf_frames import _region
	T = 10
	frames, row0, col0, time, quality, cat, targets, _ = _region(T=T)
	return frames, row0, col0, time, quality, cat, targets, np.full(T, 1e-4)


def _plugin_pos_corr(ctx, tmp_path, frames, row0, col0, time, timecorr, quality, cat, targets, mk):
	from photometry_amd.plugins import AperturePhotometry
	from photometry_amd.source import MemoryStampSource
	T = len(time)
	src = MemoryStampSource(frames, row0, col0, time, timecorr, np.arange(T), quality, cat, targets=targets, movement=mk)
	out = []
	with warnings.catch_warnings():
		warnings.simplefilter('ignore', RuntimeWarning)
		for sid in targets['starid']:
			with AperturePhotometry(int(sid), src, str(tmp_path), ctx=ctx) as pho:
				out.append(np.array(pho.lightcurve['pos_corr']))
	return np.stack(out)


def test_tessphot_frames_movement(ctx, tmp_path):
	from photometry_amd import pipeline, tessphot_frames
	from photometry_amd.tessphot import tessphot_frames_pipelined
	from photometry_amd.motion import MovementKernel
	from test_gpu_wcs import _header
	frames, row0, col0, time, quality, cat, targets, timecorr = _aperture_region()
	T, n = len(time), len(targets['starid'])
	stack = pipeline.FrameStack(ctx, {k: np.moveaxis(v, 2, 0) for k, v in frames.items()}, row0, col0)
	plain = tessphot_frames(ctx, stack, targets, cat, time, quality)
	assert plain.pos_corr is None
	n_lc = 0
	for mode in ('translation', 'euclidian', 'affine'):
		kern = _rotating_series(mode, time) if mode != 'translation' else np.column_stack((0.1 * np.sin(np.arange(T)), 0.2 * np.cos(np.arange(T))))
		mk = mp.loaded(mode, time - timecorr, kern, ctx=ctx)
		res = tessphot_frames(ctx, stack, targets, cat, time, quality, movement=mk, timecorr=timecorr)
		exp = _plugin_pos_corr(ctx, tmp_path, frames, row0, col0, time, timecorr, quality, cat, targets, mk)
		assert res.pos_corr.shape == (n, T, 2) == exp.shape
		if mode == 'translation':
			np.testing.assert_array_equal(res.pos_corr, exp)
		else:
			np.testing.assert_allclose(res.pos_corr, exp, rtol=0, atol=mp.JITTER_ATOL)
			assert np.ptp(res.pos_corr[:, 1, 0]) > 0.1
		for i in range(n):
			a, b = plain[i], res[i]
			assert a.status == b.status and a._details.keys() == b._details.keys()
			if a.lightcurve is None:
				assert b.lightcurve is None
				continue
			n_lc += 1
			assert 'pos_corr' not in a.lightcurve and set(b.lightcurve) == set(a.lightcurve) | {'pos_corr'}
			np.testing.assert_array_equal(b.lightcurve['pos_corr'], res.pos_corr[i])
			for key in a.lightcurve:
				np.testing.assert_array_equal(a.lightcurve[key], b.lightcurve[key])
			np.testing.assert_array_equal(a.final_phot_mask, b.final_phot_mask)
	assert n_lc >= 3 * (n // 2)
	# the pipelined entry gives every batch its own pos_corr
	halves = [{k: np.asarray(v)[:4] for k, v in targets.items()}, {k: np.asarray(v)[4:] for k, v in targets.items()}]
	got = list(tessphot_frames_pipelined(ctx, stack, halves, cat, time, quality, movement=mk, timecorr=timecorr))
	np.testing.assert_array_equal(np.concatenate([g.pos_corr for g in got]), res.pos_corr)
	# a 'wcs' kernel: both sides run on the device, every position a batch of its own
	hdrs = [_header(crpix=(300.0, 150.0), rot=60.0 / 3600 * np.sin(k)) for k in range(T)]
	hdrs[4] = ''
	mw = MovementKernel('wcs', wcs_ref=hdrs[0], ctx=ctx)
	mw.load_series(time - timecorr, hdrs)
	res = tessphot_frames(ctx, stack, targets, cat, time, quality, movement=mw, timecorr=timecorr)
	exp = _plugin_pos_corr(ctx, tmp_path, frames, row0, col0, time, timecorr, quality, cat, targets, mw)
	np.testing.assert_array_equal(res.pos_corr, exp)
	assert np.abs(exp).max() > 0.01


def test_refusals_without_a_launch(ctx):
	from photometry_amd._lib import TessphotError
	from photometry_amd.motion import MovementKernel
	from photometry_amd import pipeline
	times, kernels = mp.series('euclidian')
	mk = mp.loaded('euclidian', times, kernels, ctx=ctx)
	code, S, d_t, d_k, d_f, d_l = mk.device_series(ctx)
	T, n = 8, 4
	d_q = ctx.array(times[:T].copy())
	d_xy = ctx.array(mp.positions(n))
	d_base = ctx.array(np.zeros(n, dtype='float32'))
	d_oi = ctx.array(np.arange(n, dtype='int64'))
	fill = np.full((n, T), SENTINEL)
	d_pc, d_pr, d_out = ctx.array(fill), ctx.array(fill), ctx.array(np.full((T, 3), SENTINEL))

	def positions(code=code, S=S, T=T, n=n, pitch=T, single=0, xy=d_xy.ptr):
		return ctx.lib.tp_motion_star_positions(ctx.handle, code, S, d_t.ptr, d_k.ptr, d_f.ptr, d_l.ptr, T, d_q.ptr, n, xy, single, d_base.ptr, d_base.ptr,
			d_oi.ptr, n, d_pc.ptr, d_pr.ptr, pitch, None)

	def interpolate(code=code, S=S, T=T, out=d_out.ptr):
		return ctx.lib.tp_motion_interpolate(ctx.handle, code, S, d_t.ptr, d_k.ptr, d_f.ptr, d_l.ptr, T, d_q.ptr, out)

	ctx.profile(True)
	ctx.profile_reset()
	for bad in (dict(S=1), dict(T=-1), dict(pitch=T - 1), dict(n=-1), dict(code=4), dict(code=-1), dict(single=2), dict(xy=None)):
		with pytest.raises(TessphotError):
			ctx._check(positions(**bad))
	for bad in (dict(S=1), dict(T=-1), dict(code=7), dict(out=None)):
		with pytest.raises(TessphotError):
			ctx._check(interpolate(**bad))
	ctx.sync()
	launched = {name: v[0] for name, v in ctx.profile_report().items() if name in ('tp_motion_interp_kernel', 'tp_motion_positions_kernel')}
	assert launched == {}
	for a in (d_pc, d_pr, d_out):
		assert np.all(a.to_host() == SENTINEL)
	# the same arguments, valid: both kernels run
	ctx._check(positions())
	ctx._check(interpolate())
	ctx.sync()
	launched = {name: v[0] for name, v in ctx.profile_report().items() if name in ('tp_motion_interp_kernel', 'tp_motion_positions_kernel')}
	ctx.profile(False)
	assert launched == {'tp_motion_interp_kernel': 2, 'tp_motion_positions_kernel': 1}
	assert not np.any(d_pc.to_host() == SENTINEL) and not np.any(d_out.to_host() == SENTINEL)
	# an unknown warp mode is refused by the host layer
	with pytest.raises(ValueError):
		MovementKernel(warpmode='homography')
	mk.warpmode = 'homography'
	with pytest.raises(ValueError):
		mk.jitter_many(times[:2], [1.0], [2.0])
	with pytest.raises(ValueError):
		pipeline.linpsf_frames(ctx, SimpleNamespace(n_cad=2), {'starid': np.arange(1)}, {}, times[:2], None, None, movement=mk)
