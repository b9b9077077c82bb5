# -*- coding: utf-8 -*-
"""
The image movement kernels on the device (csrc/motion.hip, photometry_amd/motion.py) against the CPU restatement
(tests/motion_common.py): the prepared images, the ECC kernels and iteration counts of the three warp modes, the known answers of
shifted star fields, reproducibility, failing frames, and the path from the prepare stage into LinPSF photometry.
"""
import logging
import numpy as np
import pytest
from scipy.special import erf
import motion_common as mc

pytestmark = pytest.mark.gpu

# device prepare against prepare_flux, absolute, in float32 ulps of 1.0 (the prepared values are ~1)
PREPARE_ULPS = 4
KNOWN_ANSWER_TOL = {'translation': 0.01, 'euclidian': 0.01, 'affine': 0.015}
# the end-to-end region carries photon noise and an estimated background: measured worst error 0.031 px
END_TO_END_TOL = 0.05


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _stack(R, C, shifts, seed=11, n_stars=None):
	n_stars = n_stars or max(30, R * C // 2000)
	return np.stack([mc.star_field(R, C, shift=s, seed=seed, n_stars=n_stars) for s in shifts])


def test_prepare_matches_restatement(ctx):
	from photometry_amd import motion
	rng = np.random.default_rng(3)
	frames = _stack(2048, 2048, [(0.0, 0.0), (0.21, -0.37)])
	frames += rng.normal(0, 3.0, frames.shape).astype('float32')
	frames[1, 100, 200] = np.nan
	frames[1, 0, 7] = np.nan
	dev = motion.prepare_frames(ctx, frames).to_host()
	for k in range(len(frames)):
		ref = mc.prepare_flux(frames[k])
		d = np.abs(dev[k].astype('float64') - ref)
		ulps = d.max() / np.spacing(np.float32(1.0))
		print(f"frame {k}: max |device - prepare_flux| = {d.max():.3g} ({ulps:.2f} ulp of 1.0), bit-exact {np.mean(d == 0):.4f}")
		assert ulps <= PREPARE_ULPS
		np.testing.assert_array_equal(dev[k] == 0, ref == 0)


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
def test_ecc_matches_restatement(ctx, mode):
	from photometry_amd import motion
	rng = np.random.default_rng({'translation': 1, 'euclidian': 2, 'affine': 3}[mode])
	shifts = [(0.0, 0.0)] + [tuple(rng.uniform(-0.5, 0.5, 2)) for _ in range(15)]
	frames = _stack(512, 512, shifts)
	res = motion.movement_kernels_frames(ctx, frames, 0, warpmode=mode)
	prep = [mc.prepare_flux(f) for f in frames]
	iters = []
	for k in range(len(frames)):
		kern, rho, it, status = mc.ecc(prep[0], prep[k], mode)
		assert res['status'][k] == status == mc.CONVERGED, (k, res['status'][k], status)
		assert res['iterations'][k] == it, (k, res['iterations'][k], it)
		np.testing.assert_allclose(res['kernels'][k], kern, rtol=0, atol=1e-5)
		np.testing.assert_allclose(res['rho'][k], rho, rtol=1e-9)
		true = np.asarray(shifts[k])
		got = res['kernels'][k][[2, 5]] if mode == 'affine' else res['kernels'][k][:2]
		assert np.abs(got - true).max() < KNOWN_ANSWER_TOL[mode], (k, got, true)
		iters.append(it)
	print(mode, "iterations:", np.bincount(iters))


def test_ecc_full_frame(ctx):
	from photometry_amd import motion
	shifts = [(0.0, 0.0), (-0.31, 0.42)]
	frames = _stack(2048, 2048, shifts, n_stars=1500)
	res = motion.movement_kernels_frames(ctx, frames, 0, warpmode='translation')
	prep0, prep1 = mc.prepare_flux(frames[0]), mc.prepare_flux(frames[1])
	kern, rho, it, status = mc.ecc(prep0, prep1, 'translation')
	assert res['iterations'][1] == it and res['status'][1] == status
	np.testing.assert_allclose(res['kernels'][1], kern, rtol=0, atol=1e-5)
	assert np.abs(res['kernels'][1] - shifts[1]).max() < KNOWN_ANSWER_TOL['translation']
	assert res['iterations'][0] == 1 or np.abs(res['kernels'][0]).max() < 1e-5


def test_two_runs_bit_identical(ctx):
	from photometry_amd import motion
	rng = np.random.default_rng(9)
	frames = _stack(384, 320, [(0.0, 0.0)] + [tuple(rng.uniform(-0.5, 0.5, 2)) for _ in range(7)])
	for mode in ('translation', 'affine'):
		a = motion.movement_kernels_frames(ctx, frames, 0, warpmode=mode)
		b = motion.movement_kernels_frames(ctx, frames, 0, warpmode=mode, chunk_bytes=3 * 384 * 320 * 4)   # other chunks, same series
		for key in ('kernels', 'rho', 'iterations', 'status'):
			np.testing.assert_array_equal(a[key], b[key])


def test_failed_frames_are_nan_and_isolated(ctx, caplog):
	from photometry_amd import motion
	frames = _stack(256, 256, [(0.0, 0.0), (0.2, 0.1), (0.0, 0.0), (0.0, 0.0), (-0.3, 0.25)])
	frames[2] = 42.0           # flat
	frames[3] = np.nan         # all NaN
	with caplog.at_level(logging.ERROR, logger='photometry_amd.motion'):
		res = motion.movement_kernels_frames(ctx, frames, 0)
	assert np.all(np.isnan(res['kernels'][2:4]))
	assert set(res['status'][2:4]) <= {motion.STATUS_FAILED_NAN, motion.STATUS_FAILED_LAMBDA}
	assert sum('Could not find transform' in r.getMessage() for r in caplog.records) == 2
	alone = motion.movement_kernels_frames(ctx, frames[[0, 1, 4]], 0)
	np.testing.assert_array_equal(res['kernels'][[0, 1, 4]], alone['kernels'])
	np.testing.assert_array_equal(res['iterations'][[0, 1, 4]], alone['iterations'])
	# calc_kernel of one frame: the reference's NaN kernel on failure, a list otherwise
	mk = motion.MovementKernel('translation', image_ref=frames[0], ctx=ctx)
	assert np.all(np.isnan(mk.calc_kernel(frames[2])))
	np.testing.assert_array_equal(mk.calc_kernel(frames[4]), alone['kernels'][2])


def _drift_region(T=12, R=128, C=128, seed=21):
	rng = np.random.default_rng(seed)
	row0, col0 = 300, 500
	n = 60
	rows = rng.uniform(6, R - 6, n)
	cols = rng.uniform(6, C - 6, n)
	tmag = rng.uniform(8.5, 13.0, n)
	jitter = rng.uniform(-0.35, 0.35, (T, 2))
	rr, cc = np.arange(R), np.arange(C)
	raw = np.empty((T, R, C), dtype='float32')
	err = np.empty((T, R, C), dtype='float32')
	sig = 0.8 * np.sqrt(2)
	for k in range(T):
		img = np.zeros((R, C))
		for r, c, m in zip(rows, cols, tmag):
			pr = 0.5 * (erf((rr + 0.5 - (r + jitter[k, 1])) / sig) - erf((rr - 0.5 - (r + jitter[k, 1])) / sig))
			pc = 0.5 * (erf((cc + 0.5 - (c + jitter[k, 0])) / sig) - erf((cc - 0.5 - (c + jitter[k, 0])) / sig))
			img += 10**(-0.4 * (m - 20.451)) * np.outer(pr, pc)
		nz = np.sqrt(img + 100.0)
		raw[k] = img + 100.0 + rng.normal(size=img.shape) * nz
		err[k] = nz
	time = 1500.0 + np.arange(T) * 1800.0 / 86400.0
	quality = np.zeros(T, dtype='int32')
	ref = 5
	quality[2] = 4
	# the catalogue holds the positions in the reference frame; the kernels are the shifts relative to it
	cat = {'starid': np.arange(n, dtype='int64') + 1001, 'tmag': tmag.astype('float32'),
		'row': (rows + row0 + jitter[ref, 1]).astype('float32'), 'column': (cols + col0 + jitter[ref, 0]).astype('float32')}
	bright = np.argsort(tmag)[:6]
	targets = {'starid': cat['starid'][bright], 'tmag': tmag[bright], 'row': cat['row'][bright].astype('float64'),
		'column': cat['column'][bright].astype('float64')}
	return raw, err, time, quality, cat, targets, jitter - jitter[ref], row0, col0, ref


def test_prepare_frames_into_linpsf(ctx, tmp_path):
	from photometry_amd import prepare, pipeline, motion, psf as hpsf, simulate
	from photometry_amd.plugins import LinPSFPhotometry
	from photometry_amd.source import MemoryStampSource
	raw, err, time, quality, cat, targets, truth, row0, col0, ref = _drift_region()
	T = len(time)
	out = prepare.prepare_frames(ctx, ctx.array(raw), ctx.array(err), quality, calc_movement_kernel=True, reference_time=time[ref] + 0.001,
		time=time)
	assert out['movement_kernel_ref_frame'] == ref
	kern = out['movement_kernel']
	assert kern.shape == (T, 2) and kern.dtype == np.float64
	print("recovered - true shift: max", np.abs(kern - truth).max())
	assert np.abs(kern - truth).max() < END_TO_END_TOL
	with pytest.raises(RuntimeError):
		prepare.prepare_frames(ctx, ctx.array(raw), ctx.array(err), quality, calc_movement_kernel=True, ref_frame=2)
	mk = motion.MovementKernel('translation')
	mk.load_series(time, kern)
	host = {k: out[k].to_host() for k in ('images', 'images_err', 'backgrounds')}
	stack = pipeline.FrameStack(ctx, host, row0, col0)
	prf = simulate.synthetic_prf(seed=3)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	timecorr = np.zeros(T)
	with pytest.raises(ValueError):
		pipeline.linpsf_frames(ctx, stack, targets, cat, time, quality, model, jitter=truth, movement=mk)
	f_mov = pipeline.linpsf_frames(ctx, stack, targets, cat, time, quality, model, movement=mk, timecorr=timecorr).flux
	np.testing.assert_array_equal(f_mov, pipeline.linpsf_frames(ctx, stack, targets, cat, time, quality, model, jitter=kern).flux)
	f_true = pipeline.linpsf_frames(ctx, stack, targets, cat, time, quality, model, jitter=truth).flux
	f_none = pipeline.linpsf_frames(ctx, stack, targets, cat, time, quality, model).flux
	d_mov = np.nanmedian(np.abs(f_mov / f_true - 1))
	d_none = np.nanmedian(np.abs(f_none / f_true - 1))
	print(f"median |flux / flux(true shifts) - 1|: movement kernels {d_mov:.2e}, no shifts {d_none:.2e}")
	assert d_mov < 5e-3 and d_mov < 0.2 * d_none
	# the plugin over a MemoryStampSource with the same kernels: pos_corr is the series, the fluxes those of the same shifts as jitter
	frames_rct = {k: np.moveaxis(v, 0, 2) for k, v in host.items()}
	with pytest.raises(ValueError):
		MemoryStampSource(frames_rct, row0, col0, time, timecorr, np.arange(T), quality, cat, jitter=kern, movement=mk)
	src_m = MemoryStampSource(frames_rct, row0, col0, time, timecorr, np.arange(T), quality, cat, targets=targets, prf=model, movement=mk)
	src_j = MemoryStampSource(frames_rct, row0, col0, time, timecorr, np.arange(T), quality, cat, targets=targets, prf=model, jitter=kern)
	for i in range(2):
		sid = int(targets['starid'][i])
		with LinPSFPhotometry(sid, src_m, str(tmp_path), ctx=ctx) as pm, LinPSFPhotometry(sid, src_j, str(tmp_path), ctx=ctx) as pj:
			pm.do_photometry()
			pj.do_photometry()
			np.testing.assert_array_equal(pm.lightcurve['pos_corr'], mk.jitter(time - timecorr, targets['column'][i], targets['row'][i]))
			np.testing.assert_allclose(pm.lightcurve['pos_corr'], kern, rtol=0, atol=1e-12)   # interp1d at the nodes
			np.testing.assert_allclose(pm.lightcurve['flux'], pj.lightcurve['flux'], rtol=1e-5)
