# -*- coding: utf-8 -*-
"""
The image movement kernels on the device (csrc/motion.hip, photometry_amd/motion.py) against the CPU restatement
(tests/motion_common.py): the prepared images, the ECC kernels and iteration counts of the three warp modes, the known answers of
shifted star fields, reproducibility, failing frames, and the path from the prepare stage into LinPSF photometry.

The second half holds the same kernels to the restatement off their tile grids (prepare / blur 16 x 64, iteration 32 x 128): ragged and
tiny frames, one iteration at a time, warps that push a band of pixels out of the frame, rotations and affine matrices, iteration caps
inside every poll interval of the host loop, a padded frame stride and a reference frame in the middle of the stack.  The cases and
their input conditions live in tests/motion_common.py; tests/test_motion_host.py asserts the conditions on the restatement alone.
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


# ---- off the tile grid ---------------------------------------------------------------------------------------------------------------

def _ids(v):
	return v if isinstance(v, str) else f"{v[0]}x{v[1]}"


def _same_result(res, k, ref, mode, label):
	"""Frame ``k`` of a device result against the restatement's ``(kernel, rho, iterations, status)`` at the tolerances of DESIGN.md
	section 9; returns (worst kernel difference, relative rho difference) for the record."""
	kern, rho, it, status = ref[:4]
	assert res['status'][k] == status, (label, res['status'][k], status)
	assert res['iterations'][k] == it, (label, res['iterations'][k], it)
	if status >= mc.FAILED_NAN:
		assert np.all(np.isnan(res['kernels'][k])), label
		assert np.isnan(res['rho'][k]) == np.isnan(rho), label
		if not np.isnan(rho):
			np.testing.assert_allclose(res['rho'][k], rho, rtol=1e-9, err_msg=str(label))
		return 0.0, 0.0
	dk = np.abs(res['kernels'][k] - kern).max()
	dr = abs(res['rho'][k] - rho) / abs(rho)
	print(f"  {label}: status {status} iterations {it}: max |kernel - restatement| = {dk:.3g}, |rho - restatement| / |rho| = {dr:.3g}")
	np.testing.assert_allclose(res['kernels'][k], kern, rtol=0, atol=1e-5, err_msg=str(label))
	np.testing.assert_allclose(res['rho'][k], rho, rtol=1e-9, err_msg=str(label))
	return dk, dr


@pytest.mark.parametrize('shape', mc.RAGGED_SHAPES, ids=_ids)
def test_prepare_ragged_matches_restatement(ctx, shape):
	"""The tails of the min / max and prepare kernels and the clamped, reflected halo of a partly filled tile, NaN pixels on every edge."""
	from photometry_amd import motion
	frames = mc.ragged_stack(*shape)
	dev = motion.prepare_frames(ctx, frames).to_host()
	assert dev.shape == frames.shape
	worst = 0.0
	for k in range(len(frames)):
		ref = mc.prepare_flux(frames[k])
		ulps = np.abs(dev[k].astype('float64') - ref).max() / np.spacing(np.float32(1.0))
		worst = max(worst, ulps)
		assert ulps <= PREPARE_ULPS, (shape, k, ulps)
		np.testing.assert_array_equal(dev[k] == 0, ref == 0)
	np.testing.assert_array_equal(dev[2:], 0)
	print(f"prepare {shape}: worst |device - prepare_flux| = {worst:.2f} ulp of 1.0")


@pytest.mark.parametrize('mode', mc.MODES)
@pytest.mark.parametrize('shape', mc.ONE_STEP_SHAPES, ids=_ids)
def test_one_iteration_matches_restatement(ctx, shape, mode):
	"""
	Exactly one iteration from the same prepared images: the blur's mirrored halo, the corner gradients, the tile tails and the moment
	sums with nothing averaged away.  The first iteration's mask is the whole frame (identity warp), so the pairs whose warp leaves the
	frame are compared again after MASK_STEPS iterations with eps = 0, where the mask count is at most MASK_SHARE of the frame.
	"""
	from photometry_amd import motion
	names, flags, prep = mc.one_step_prepared(*shape)
	d_prep = ctx.array(prep)
	res = motion.ecc_prepared(ctx, d_prep.slice0(0, 1), d_prep, mode, number_of_iterations=1)
	worst = [0.0, 0.0]
	for k, name in enumerate(names):
		ref = mc.ecc_step(prep[0], prep[k], mode)
		assert ref[2] == 1
		worst = np.maximum(worst, _same_result(res, k, ref, mode, (shape, mode, name, 1)))
	more = motion.ecc_prepared(ctx, d_prep.slice0(0, 1), d_prep, mode, number_of_iterations=mc.MASK_STEPS, termination_eps=0.0)
	for k, name in enumerate(names):
		if flags[k]:
			ref = mc.ecc(prep[0], prep[k], mode, max_iter=mc.MASK_STEPS, eps=0.0, history=True)
			assert ref[4][-1]['N'] <= mc.MASK_SHARE * shape[0] * shape[1], (name, ref[4][-1]['N'])
			assert (ref[2], ref[3]) == (mc.MASK_STEPS, mc.CAP_REACHED)
			worst = np.maximum(worst, _same_result(more, k, ref, mode, (shape, mode, name, mc.MASK_STEPS)))
	print(f"one step {shape} {mode}: worst kernel difference {worst[0]:.3g}, worst relative rho difference {worst[1]:.3g}")


@pytest.mark.parametrize('shape,mode', mc.TINY_CASES, ids=_ids)
def test_one_iteration_tiny_frames(ctx, shape, mode):
	"""Frames smaller than one tile, down to the 3 x 3 the C entry accepts: one smooth star, one step, a conditioned Hessian."""
	from photometry_amd import motion
	prep = mc.tiny_prepared(*shape)
	d_prep = ctx.array(prep)
	res = motion.ecc_prepared(ctx, d_prep.slice0(0, 1), d_prep, mode, number_of_iterations=1)
	for k in range(2):
		ref = mc.ecc_step(prep[0], prep[k], mode, history=True)
		assert ref[4][0]['cond'] <= mc.TINY_MAX_COND and ref[4][0]['N'] >= 2 * mc.N_PARAMS[mode]
		assert (ref[2], ref[3]) == (1, mc.CAP_REACHED)
		_same_result(res, k, ref, mode, (shape, mode, k))


@pytest.mark.parametrize('mode', mc.MODES)
@pytest.mark.parametrize('shape', mc.CONVERGED_SHAPES, ids=_ids)
def test_converged_ragged_general_warps(ctx, shape, mode):
	"""Converged parity on ragged frames: large shifts (N well below R * C), rotations, scale and shear."""
	from photometry_amd import motion
	names, warps, known, frames = mc.converged_stack(shape, mode)
	res = motion.movement_kernels_frames(ctx, frames, 0, warpmode=mode)
	prep = [mc.prepare_flux(f) for f in frames]
	worst = [0.0, 0.0]
	for k, name in enumerate(names):
		ref = mc.ecc(prep[0], prep[k], mode)
		assert ref[3] == mc.CONVERGED
		worst = np.maximum(worst, _same_result(res, k, ref, mode, (shape, mode, name)))
		if known[k]:
			err = np.abs(res['kernels'][k] - mc.warp_to_kernel(warps[k], mode)).max()
			assert err < KNOWN_ANSWER_TOL[mode], (shape, mode, name, err)
	print(f"converged {shape} {mode}: worst kernel difference {worst[0]:.3g}, worst relative rho difference {worst[1]:.3g}")


def test_reference_frame_in_the_middle(ctx):
	from photometry_amd import motion
	frames = mc.ref_middle_stack()
	ref, mode = mc.REF_MIDDLE['ref_frame'], mc.REF_MIDDLE['mode']
	res = motion.movement_kernels_frames(ctx, frames, ref, warpmode=mode)
	prep = [mc.prepare_flux(f) for f in frames]
	for k in range(len(frames)):
		_same_result(res, k, mc.ecc(prep[ref], prep[k], mode), mode, ('ref_frame', ref, k))
		true = np.subtract(mc.REF_MIDDLE['shifts'][k], mc.REF_MIDDLE['shifts'][ref])
		assert np.abs(res['kernels'][k] - true).max() < KNOWN_ANSWER_TOL[mode]


@pytest.mark.parametrize('mode', mc.MODES)
def test_iteration_caps_and_poll_loop(ctx, mode):
	"""eps = 0: every frame runs to the cap, which falls before the first poll (1, 3) and inside the second, third and fourth interval
	of the host loop (5, 13, 37); a cap of 0 leaves the identity warp and rho = -1.

	Both sides start from the restatement's prepared images.  Far from the maximum rho is first order in the pixels: with the device's
	own prepared images (2 ulp of float32 from prepare_flux, the rounding of log10) the rho of the 3.7 px pair after one iteration,
	0.546, was measured 3.5e-9 off in relative terms, against 2e-16 from equal pixels -- the prepare stage's tolerance, not the ECC's.
	"""
	from photometry_amd import motion
	frames = mc.cap_stack()
	prep = [mc.prepare_flux(f) for f in frames]
	d_prep = ctx.array(np.stack(prep))
	hist = [mc.ecc(prep[0], p, mode, max_iter=max(mc.CAPS), eps=0.0, history=True)[4] for p in prep]
	for cap in mc.CAPS:
		res = motion.ecc_prepared(ctx, d_prep.slice0(0, 1), d_prep, mode, number_of_iterations=cap, termination_eps=0.0)
		worst = [0.0, 0.0]
		for k in range(len(frames)):
			if cap == 0:
				ref = (mc.warp_to_kernel(np.eye(2, 3), mode), -1.0, 0, mc.CAP_REACHED)
				np.testing.assert_array_equal(res['kernels'][k], ref[0])
				assert res['rho'][k] == -1.0
			elif cap == max(mc.CAPS) or k == 1:
				ref = mc.ecc(prep[0], prep[k], mode, max_iter=cap, eps=0.0)
			else:
				# a cap only cuts the series (asserted in tests/test_motion_host.py): the restatement's state after ``cap`` iterations
				assert len(hist[k]) == max(mc.CAPS)
				ref = (mc.warp_to_kernel(hist[k][cap - 1]['warp'], mode), hist[k][cap - 1]['rho'], cap, mc.CAP_REACHED)
			assert (ref[2], ref[3]) == (cap, mc.CAP_REACHED)
			worst = np.maximum(worst, _same_result(res, k, ref, mode, (mode, 'cap', cap, k)))
		print(f"cap {cap} {mode}: worst kernel difference {worst[0]:.3g}, worst relative rho difference {worst[1]:.3g}")


@pytest.mark.parametrize('mode', mc.MODES)
def test_mixed_chunk_frozen_capped_failed(ctx, mode, caplog):
	"""One chunk with a frame that converges in the first poll interval, one in the second, one that is capped and two that fail; the
	same frames alone and in chunks of one and of two frames give the same bits."""
	from photometry_amd import motion
	frames = mc.mixed_stack()
	R, C = frames.shape[1:]
	prep = [mc.prepare_flux(f) for f in frames]
	with caplog.at_level(logging.CRITICAL, logger='photometry_amd.motion'):
		res = motion.movement_kernels_frames(ctx, frames, 0, warpmode=mode, number_of_iterations=mc.MIXED_CAP)
		seen = set()
		for k in range(len(frames)):
			ref = mc.ecc(prep[0], prep[k], mode, max_iter=mc.MIXED_CAP)
			seen.add(ref[3])
			_same_result(res, k, ref, mode, (mode, 'mixed', k))
		assert {mc.CONVERGED, mc.CAP_REACHED} <= seen and max(seen) >= mc.FAILED_NAN
		for n in (1, 2):
			other = motion.movement_kernels_frames(ctx, frames, 0, warpmode=mode, number_of_iterations=mc.MIXED_CAP, chunk_bytes=n * R * C * 4)
			for key in ('kernels', 'warp', 'rho', 'iterations', 'status'):
				np.testing.assert_array_equal(res[key], other[key])
		for k in range(1, len(frames)):
			alone = motion.movement_kernels_frames(ctx, frames[[0, k]], 0, warpmode=mode, number_of_iterations=mc.MIXED_CAP)
			for key in ('kernels', 'warp', 'rho', 'iterations', 'status'):
				np.testing.assert_array_equal(res[key][[0, k]], alone[key])


@pytest.mark.parametrize('mode', mc.MODES)
def test_padded_frame_stride(ctx, mode):
	"""``frame_stride > rows * cols`` through the C entries: padding of NaN and of 1e30 between the frames changes no bit."""
	from photometry_amd import motion
	R, C = mc.PAD_SHAPE
	n_pix, stride = R * C, R * C + mc.PAD
	names, warps, known, frames = mc.converged_stack(mc.PAD_SHAPE, mode)
	T = len(frames)
	contiguous = motion.prepare_frames(ctx, frames)
	prepared = contiguous.to_host()
	chunk_bytes = 2 * n_pix * 4
	ref = motion.ecc_prepared(ctx, contiguous.slice0(0, 1), contiguous, mode, chunk_bytes=chunk_bytes)
	assert np.all(ref['status'] == motion.STATUS_CONVERGED)
	for fill in (np.nan, 1e30):
		padded = np.full((T, stride), fill, dtype='float32')
		padded[:, :n_pix] = frames.reshape(T, n_pix)
		d_pad = ctx.array(padded)
		d_out = ctx.empty((T, R, C), 'float32')
		d_out.fill_bytes(0xff)
		ctx._check(ctx.lib.tp_motion_prepare(ctx.handle, d_pad.ptr, T, R, C, stride, d_out.ptr))
		np.testing.assert_array_equal(d_out.to_host(), prepared)
		padded[:, :n_pix] = prepared.reshape(T, n_pix)
		d_pad = ctx.array(padded)
		d_warp, d_rho = ctx.empty((T, 6), 'float64'), ctx.empty((T,), 'float64')
		d_iters, d_status = ctx.empty((T,), 'int32'), ctx.empty((T,), 'int32')
		ctx._check(ctx.lib.tp_motion_ecc(ctx.handle, contiguous.ptr, d_pad.ptr, T, R, C, stride, mc.N_PARAMS[mode], 10000, 1e-6, chunk_bytes,
			d_warp.ptr, d_rho.ptr, d_iters.ptr, d_status.ptr))
		np.testing.assert_array_equal(d_warp.to_host().reshape(T, 2, 3), ref['warp'])
		np.testing.assert_array_equal(d_rho.to_host(), ref['rho'])
		np.testing.assert_array_equal(d_iters.to_host(), ref['iterations'])
		np.testing.assert_array_equal(d_status.to_host(), ref['status'])


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
