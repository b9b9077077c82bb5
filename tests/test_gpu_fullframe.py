# -*- coding: utf-8 -*-
"""
GPU parity of the full-frame prepare-stage arithmetic (B1 fit_background for a plain image, B2 / B3 / A1 on images) against
the oracle, and the reference's own known answer for the background estimator (tests/test_background.py:36-54: a constant
2048 x 2048 image of 1000 comes back as 1000 with nothing masked).

B1 is float64 statistics on float32 pixels summed in different orders: the float32 background agrees to 1e-6 relative.
B2, B3 and A1 are bit-exact (A1: float64 sums of float32 values in frame order on both sides).
"""
import numpy as np
import pytest
import radial_common

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _frames(T, R, C, seed):
	rng = np.random.default_rng(seed)
	yy, xx = np.mgrid[0:R, 0:C]
	sky = 100 + 0.03 * xx + 0.015 * yy + 5 * np.sin(xx / 90.0)
	f = np.empty((T, R, C), dtype='float32')
	for k in range(T):
		img = sky * (1 + 0.02 * np.sin(k)) + rng.normal(0, 3, (R, C))
		for _ in range(40):     # stars
			r, c = rng.integers(0, R), rng.integers(0, C)
			img[max(r-2, 0):r+3, max(c-2, 0):c+3] += rng.uniform(500, 90000)
		f[k] = img
	f[0, 10:20, 30:40] = np.nan
	f[1, 64:128, 0:64] = -5.0            # a box that is entirely masked -> filled from its neighbours
	if T > 2:
		f[2, 128:192, 64:128][::2] = np.inf  # half masked: still kept (<= 50 %)
		f[2, 128:192, 128:192][:33] = np.nan # more than half masked: dropped
	return f


def test_fit_background_reference_known_answer(ctx):
	from photometry_amd import prepare
	img = np.full((1, 2048, 2048), 1000, dtype='float32')
	bkg, mesh, nmasked = prepare.fit_background_frames(ctx, ctx.array(img), return_mask=True)
	b = bkg.to_host()
	assert b.shape == (1, 2048, 2048) and np.all(np.isfinite(b))
	assert not nmasked.any(), "Nothing should be masked out"
	np.testing.assert_allclose(b, 1000)


def test_fit_background_large_mesh(ctx):
	"""A mesh above the 2048 cells of rounds 4-5 (here 88 x 81 = 7128 cells of 16 pixels: the finishing kernel's work arrays are
	sized at launch, up to 8192 cells) against the oracle with the same box; more cells than that are refused, not mangled."""
	from photometry_amd import prepare
	from oracle import backgrounds as ob
	R, C, box = 1408, 1296, 16
	f = _frames(2, R, C, seed=5)[:1]
	f[0, 400:432, 600:632] = np.nan          # four whole cells masked: filled from their neighbours
	bkg, mesh, nmasked = prepare.fit_background_frames(ctx, ctx.array(f), box=box, return_mask=True)
	mask = ob.stamp_mask(f[0])
	ref_mesh, ref_nm = ob.mesh_statistics(f[0], mask, box=box)
	np.testing.assert_array_equal(nmasked[0], ref_nm)
	np.testing.assert_allclose(mesh[0], ref_mesh, rtol=1e-9, equal_nan=True)
	ref = ob.mesh_to_background(ref_mesh, ref_nm, (R, C), box=box)
	np.testing.assert_allclose(bkg.to_host()[0], ref, rtol=1e-6)
	with pytest.raises(ValueError, match='at most 8192 cells'):
		prepare.fit_background_frames(ctx, ctx.array(f), box=8)


@pytest.mark.parametrize("T,R,C", [(3, 256, 320), (2, 200, 150)])
def test_fit_background_matches_oracle(ctx, T, R, C):
	from photometry_amd import prepare
	from oracle import backgrounds as ob
	f = _frames(T, R, C, seed=R)
	bkg, mesh, nmasked = prepare.fit_background_frames(ctx, ctx.array(f), return_mask=True)
	b = bkg.to_host()
	for k in range(T):
		mask = ob.stamp_mask(f[k])
		ref_mesh, ref_nm = ob.mesh_statistics(f[k], mask)
		np.testing.assert_array_equal(nmasked[k], ref_nm)
		np.testing.assert_allclose(mesh[k], ref_mesh, rtol=1e-9, equal_nan=True)
		ref, _ = ob.fit_background(f[k])
		np.testing.assert_allclose(b[k], ref, rtol=1e-6)
	# the estimate follows the injected sky, stars clipped away
	yy, xx = np.mgrid[0:R, 0:C]
	sky = (100 + 0.03 * xx + 0.015 * yy + 5 * np.sin(xx / 90.0)) * (1 + 0.02 * np.sin(0))
	assert np.median(np.abs(b[0] / sky - 1)) < 0.05   # a 64-pixel mesh over a sky gradient: a sanity check, not parity


def test_prepare_frames_matches_oracle(ctx):
	from photometry_amd import prepare
	from oracle import backgrounds as ob, sumimage as osum
	T, R, C = 7, 128, 192
	f = _frames(T, R, C, seed=5)
	err = np.sqrt(np.abs(np.nan_to_num(f, nan=1.0, posinf=1.0)) + 100).astype('float32')
	quality = np.zeros(T, dtype='int32'); quality[3] = 32
	flags = np.zeros((T, R, C), dtype='uint8'); flags[2, 5, 6] = 2; flags[4, 7, 8] = 1
	out = prepare.prepare_frames(ctx, ctx.array(f), ctx.array(err), quality, pixel_flags=ctx.array(flags))
	bkg = out['backgrounds'].to_host()
	# B2 / B3 / A1 from the device's own unsmoothed backgrounds would need them: recompute the chain with the oracle on the
	# device backgrounds instead (B1 is compared above)
	us = prepare.fit_background_frames(ctx, ctx.array(f), exclude=ctx.array(flags)).to_host()   # flagged pixels are masked (backgrounds.py:96-97)
	ref_bkg = np.moveaxis(ob.smooth_time(np.moveaxis(us, 0, -1), 3), -1, 0)
	np.testing.assert_array_equal(bkg, ref_bkg)
	ref_img, ref_err = ob.subtract_background(f, err, bkg, flags)
	np.testing.assert_array_equal(out['images'].to_host(), ref_img)
	np.testing.assert_array_equal(out['images_err'].to_host(), ref_err)
	ref_sum = osum.sumimage(np.moveaxis(ref_img, 0, -1), quality)
	np.testing.assert_array_equal(out['sumimage'].to_host(), ref_sum)


def test_background_shenanigans(ctx):
	"""The pixel-flag pass of the prepare stage (pixel_flags.py:61-79, prepare.py:515-622): 15 x 15 median filter of img - SumImage
	(scipy itself is the check: bit-exact), block-median mean over the reference's own frame shuffle, thresholded flags."""
	from scipy.ndimage import median_filter
	from photometry_amd import prepare
	from oracle import backgrounds as ob
	rng = np.random.default_rng(8)
	T, R, C = 50, 40, 70
	sky = rng.normal(0, 3, (T, R, C)).astype('float32')
	sky[20:30, 10:30, 20:60] += 90.0          # a scattered-light patch in ten frames: flagged there
	sky[:, 5, 5] += 5000.0                     # a star: removed by the median filter
	sumimage = np.median(sky.astype('float64'), axis=0)
	flags0 = np.zeros((T, R, C), dtype='uint8'); flags0[0, 1, 1] = 4; flags0[3, 2, 2] = 1 | 4
	d_flags = ctx.array(flags0)
	ind, mean = prepare.background_shenanigans(ctx, ctx.array(sky), ctx.array(sumimage), d_flags)
	got_ind = ind.to_host()
	for k in (0, 7, 25):
		ref = median_filter(sky[k] - sumimage, size=15)            # float64, as the reference computes it
		np.testing.assert_array_equal(got_ind[k], ref.astype('float32'))
	rflags, rind, rmean = ob.background_shenanigans_flags(sky, sumimage, flags0)
	np.testing.assert_array_equal(got_ind, rind)
	np.testing.assert_allclose(mean.to_host(), rmean, rtol=1e-13, atol=1e-13)
	got = d_flags.to_host()
	np.testing.assert_array_equal(got, rflags)
	assert (got[22] & 4).sum() > 500 and (got[40] & 4).sum() == 0 and got[3, 2, 2] == 1
	# small windows / no reference image
	small = prepare.ctypes  # noqa: F841 (keep the import used)
	out = ctx.empty((3, R, C), 'float32')
	d_sky3 = ctx.array(sky[:3])
	ctx._check(ctx.lib.tp_frames_median_filter(ctx.handle, d_sky3.ptr, 3, R, C, C, R * C, None, 5, out.ptr))
	np.testing.assert_array_equal(out.to_host()[1], median_filter(sky[1], size=5))


def test_shenanigans_mean_golden_on_device(ctx, golden_dir):
	"""The block-median mean against the reference's own statements (tests/golden/golden_shenanigans.npz), frame counts that are
	not a multiple of 25 included: a 1 x 1 "median filter" with a zero reference image hands the golden indicator through."""
	import os
	from photometry_amd import prepare
	g = np.load(os.path.join(golden_dir, 'golden_shenanigans.npz'))
	for c in range(int(g['n_cases'])):
		ind = g[f's{c}_indicator']
		T, R, C = ind.shape
		flags = ctx.zeros((T, R, C), 'uint8')
		got_ind, mean = prepare.background_shenanigans(ctx, ctx.array(ind), ctx.array(np.zeros((R, C))), flags, size=1)
		np.testing.assert_array_equal(got_ind.to_host(), ind)
		np.testing.assert_allclose(mean.to_host(), g[f's{c}_mean'], rtol=1e-15, atol=0)


def _tess_frames(T, R, C, seed):
	"""Frames of the corner of CCD (1, 1): a sky plus a glow rising with the distance from the camera centre, stars, defects."""
	from photometry_amd import prepare
	rng = np.random.default_rng(seed)
	xc, yc = prepare.CAMERA_CENTRE[(1, 1)]
	yy, xx = np.mgrid[0:R, 0:C]
	r = np.hypot(xx + 44 - xc, yy - yc)
	f = np.empty((T, R, C), dtype='float32')
	for k in range(T):
		glow = (40 + 10 * k) * np.exp((r - 2400) / 250.0)
		img = 120 + 0.02 * xx + glow + rng.normal(0, 4, (R, C))
		for _ in range(60):
			y, x = rng.integers(0, R), rng.integers(0, C)
			img[max(y-2, 0):y+3, max(x-2, 0):x+3] += rng.uniform(500, 90000)
		f[k] = img
	f[0, 5:9, 7:30] = np.nan
	f[-1, 100:164, 200:264] = -3.0
	return f


@pytest.mark.parametrize("T,R,C", [(2, 384, 448)])
def test_fit_background_tess_matches_oracle(ctx, T, R, C):
	"""
	The TESS branch (radial rings + mesh, three rounds).  A ring mode is the argmax over a 2048-point KDE grid: where two
	neighbouring grid points tie within rounding, ANY last-bit difference in the samples moves the mode by a whole grid step
	(~5e-4 in log10, ~1e-3 in the background).  The reference's own samples carry such differences from machine to machine:
	its first round takes numpy's float32 log10, a libm / SVML routine that is off by one ulp on ~40 % of its arguments.

	* Against the oracle with the device's three roundings written out (``device_arithmetic``: correctly rounded float32
	  log10, float32 storage of the two components between the rounds, fixed-point binning) every ring mode must be the same
	  grid point and the background agree to 1e-5 (north_star's tolerance).
	* Against the literal oracle (numpy's float32 log10, float64 components) the same holds except in the rings whose mode
	  sits on such a tie: at most 3 per round may differ, by one grid step.
	* The device result is reproducible bit for bit (ordered compaction, integer binning: nothing depends on arrival order).
	"""
	from photometry_amd import prepare
	from oracle import backgrounds as ob
	f = _tess_frames(T, R, C, seed=5)
	details = {}
	d_f = ctx.array(f)
	bkg = prepare.fit_background_frames(ctx, d_f, camera=1, ccd=1, details=details)
	b = bkg.to_host()
	details2 = {}
	b2 = prepare.fit_background_frames(ctx, d_f, camera=1, ccd=1, details=details2).to_host()
	assert np.array_equal(b, b2, equal_nan=True)
	for it in range(3):
		assert np.array_equal(details['s2'][it], details2['s2'][it], equal_nan=True)
	worst = worst_dev = 0.0
	for k in range(T):
		# --- the device's arithmetic restated: no tie is decided by a rounding the two sides do differently
		refd, _, interd = ob.fit_background_tess(f[k], 1, 1, full=True, device_arithmetic=True)
		for it in range(3):
			s_dev, s_ref = details['s2'][it][k], interd['s2'][it]
			assert np.array_equal(np.isnan(s_dev), np.isnan(s_ref))
			ok = ~np.isnan(s_ref)
			d = np.abs(s_dev[ok] - s_ref[ok])
			print('frame', k, 'round', it, '[device arithmetic] max ring-mode diff', float(d.max()))
			assert d.max() < 2e-5, (k, it, d)
		errd = np.abs(b[k] - refd) / np.abs(refd)
		worst_dev = max(worst_dev, float(errd.max()))
		assert errd.max() < 2e-6, (k, float(errd.max()))   # measured on 32 full frames with the round-5/6 kernels: 6.4e-7 at worst (profiles/r6_tess_flip_stats.txt)
		# --- the literal restatement of the reference
		flipped = 0
		ref, mask, inter = ob.fit_background_tess(f[k], 1, 1, full=True)
		for it in range(3):
			s_dev, s_ref = details['s2'][it][k], inter['s2'][it]
			assert np.array_equal(np.isnan(s_dev), np.isnan(s_ref))
			ok = ~np.isnan(s_ref)
			assert ok.sum() >= 30
			np.testing.assert_allclose(details['zeropoint'][it][k], inter['zeropoint'][it], rtol=1e-6)
			d = np.abs(s_dev[ok] - s_ref[ok])
			exact = d < 2e-5
			print('frame', k, 'round', it, '[literal] rings on the same grid point:', int(exact.sum()), 'of', int(ok.sum()), 'max diff', float(d.max()),
				'median diff', float(np.median(d)))
			assert exact.sum() >= ok.sum() - 3, (k, it, d)
			assert d.max() < 2e-3, (k, it, d.max())
			flipped += int(ok.sum() - exact.sum())
		err = np.abs(b[k] - ref) / np.abs(ref)
		worst = max(worst, float(err.max()))
		assert err.max() < (5e-4 if flipped else 1e-5), (k, flipped, float(err.max()))   # measured on 32 full frames (profiles/r6_tess_flip_stats.txt): 1.3e-4 at worst with a flipped ring
		# the radial component matters here: without it the corner is off by far more than the tolerance
		plain = ob.fit_background(f[k])[0]
		assert np.max(np.abs(plain - ref) / ref) > 0.01
	print('TESS background: worst relative deviation', worst_dev, '(device arithmetic restated)', worst, '(literal)')


def test_fit_background_tess_full_frames(ctx):
	"""The TESS branch on full 2048 x 2048 frames (the size the reference runs it on: 39 rings of ~10 000 pixels, a 32 x 32 mesh):
	every ring mode on the oracle's grid point and the background within 1e-5 against the oracle with the device's roundings
	written out; against the literal oracle the tie allowance of the small-frame test."""
	from photometry_amd import prepare
	from oracle import backgrounds as ob
	T, R, C = 2, 2048, 2048
	f = _tess_frames(T, R, C, seed=11)
	details = {}
	b = prepare.fit_background_frames(ctx, ctx.array(f), camera=1, ccd=1, details=details).to_host()
	for k in range(T):
		refd, _, interd = ob.fit_background_tess(f[k], 1, 1, full=True, device_arithmetic=True)
		for it in range(3):
			s_dev, s_ref = details['s2'][it][k], interd['s2'][it]
			assert np.array_equal(np.isnan(s_dev), np.isnan(s_ref)) and np.sum(~np.isnan(s_ref)) >= 30
			d = np.abs(s_dev - s_ref)[~np.isnan(s_ref)]
			print('frame', k, 'round', it, 'max ring-mode diff', float(d.max()))
			assert d.max() < 2e-5, (k, it, d)
		errd = np.abs(b[k] - refd) / np.abs(refd)
		print('frame', k, 'max relative background deviation', float(errd.max()))
		assert errd.max() < 2e-6          # profiles/r6_tess_flip_stats.txt: 6.4e-7 at worst on 32 full frames
	ref, _, inter = ob.fit_background_tess(f[0], 1, 1, full=True)
	flipped = sum(int(np.sum(np.abs(details['s2'][it][0] - inter['s2'][it]) >= 2e-5)) for it in range(3))
	err = np.abs(b[0] - ref) / np.abs(ref)
	print('literal oracle: rings off their grid point', flipped, 'max relative deviation', float(err.max()))
	assert flipped <= 9 and err.max() < (5e-4 if flipped else 1e-5)


def test_mesh_finish_and_ring_profiles_on_device(ctx):
	"""The two small device passes that replaced host numpy / scipy work in the full-frame background: the finishing of the
	low-resolution mesh (excluded cells, 3 x 3 nan-median, scipy.ndimage spline prefilter) and the ring profile (moving median,
	interpolating cubic spline in FITPACK form) -- each against the host functions that call numpy / scipy themselves."""
	from scipy import ndimage
	from scipy.interpolate import InterpolatedUnivariateSpline
	from photometry_amd import prepare
	rng = np.random.default_rng(21)
	T, ny, nx, box = 7, 32, 32, 64
	mesh = rng.normal(150, 5, (T, ny, nx))
	nm = rng.integers(0, 1000, (T, ny, nx)).astype('int32')
	nm[0, 3:9, 4:20] = 3000                       # a block of excluded cells
	nm[1, :, :] = 4096; nm[1, 10, 11] = 5         # one kept cell
	nm[2, :, :] = 4000                            # nothing kept
	mesh[3, 5, 5] = np.nan; mesh[3, 0, 0] = np.nan # non-finite statistics count as excluded
	nm[4, ::2, :] = 2500                          # every other row excluded
	nm[5, 0, :] = 2049; nm[5, :, -1] = 2049       # edges excluded (2048 = exactly 50 % is still kept)
	nm[6, 7, 7] = 2048
	coef, vmin, vmax, filt = ctx.empty((T, ny, nx), 'float64'), ctx.empty((T,), 'float64'), ctx.empty((T,), 'float64'), ctx.empty((T, ny, nx), 'float64')
	d_mesh, d_nm = ctx.array(mesh), ctx.array(nm)   # (named: a temporary's block would go back to the allocation cache before the call)
	ctx._check(ctx.lib.tp_background_mesh_finish(ctx.handle, d_mesh.ptr, d_nm.ptr, T, ny, nx, box, 50.0, 3, coef.ptr, vmin.ptr, vmax.ptr, filt.ptr))
	ref = prepare.finish_mesh(mesh, nm, box)
	got = filt.to_host()
	assert np.all(np.isnan(got[2])) and np.all(np.isnan(ref[2]))
	np.testing.assert_allclose(got, ref, rtol=1e-14, equal_nan=True)
	c = ndimage.spline_filter1d(ndimage.spline_filter1d(ref, order=3, axis=1, mode='reflect'), order=3, axis=2, mode='reflect')
	np.testing.assert_allclose(coef.to_host(), c, rtol=1e-12, atol=1e-10, equal_nan=True)
	np.testing.assert_array_equal(vmin.to_host(), np.min(ref, axis=(1, 2)))
	np.testing.assert_array_equal(vmax.to_host(), np.max(ref, axis=(1, 2)))
	# a non-square mesh and no filter
	mesh2 = rng.normal(10, 1, (2, 5, 9)); nm2 = np.zeros((2, 5, 9), dtype='int32'); nm2[0, 2, 3:6] = 4096
	coef2, f2 = ctx.empty((2, 5, 9), 'float64'), ctx.empty((2, 5, 9), 'float64')
	d_mesh2, d_nm2 = ctx.array(mesh2), ctx.array(nm2)
	ctx._check(ctx.lib.tp_background_mesh_finish(ctx.handle, d_mesh2.ptr, d_nm2.ptr, 2, 5, 9, box, 50.0, 1, coef2.ptr, vmin.ptr, vmax.ptr, f2.ptr))
	ref2 = prepare.finish_mesh(mesh2, nm2, box, filter_size=1)
	np.testing.assert_allclose(f2.to_host(), ref2, rtol=1e-14)
	# short axes: the causal initialisation of scipy's prefilter (accumulated in place) matters most here
	c2 = ndimage.spline_filter1d(ndimage.spline_filter1d(ref2, order=3, axis=1, mode='reflect'), order=3, axis=2, mode='reflect')
	np.testing.assert_allclose(coef2.to_host(), c2, rtol=1e-13)

	# ---- ring profiles
	nr = 39
	bc = 2400.0 + 15.0 * np.arange(nr) + 7.5
	s2 = 2.0 + 0.004 * np.arange(nr)[None, :] + rng.normal(0, 2e-3, (9, nr))
	s2[1, 0] = np.nan; s2[1, 17:20] = np.nan; s2[1, -1] = np.nan
	s2[2, :] = np.nan; s2[2, 5] = 2.0; s2[2, 6] = 2.1                      # two usable rings: no radial component
	s2[3, :] = np.nan; s2[3, 3:8] = [2.0, 2.1, 2.05, 2.2, 2.15]           # a short run
	s2[4, ::2] = np.nan                                                    # every other ring missing: medians fill them
	s2[5, :] = np.nan; s2[5, [4, 20, 30]] = 2.0                            # isolated rings
	for smooth in (3, 0, 5):
		K = nr + 4
		knots, coefs, nk = ctx.zeros((9, K), 'float64'), ctx.zeros((9, K), 'float64'), ctx.zeros((9,), 'int32')
		d_s2, d_bc = ctx.array(s2), ctx.array(bc)
		ctx._check(ctx.lib.tp_radial_profiles(ctx.handle, 9, nr, d_s2.ptr, d_bc.ptr, smooth, K, knots.ptr, coefs.ptr, nk.ptr))
		kn, co, n = knots.to_host(), coefs.to_host(), nk.to_host()
		for k in range(9):
			prof = prepare._move_median_central(s2[k], smooth) if smooth else s2[k]
			good = ~np.isnan(prof)
			if good.sum() < 4:
				assert n[k] == 0
				continue
			t, c, _ = InterpolatedUnivariateSpline(bc[good], prof[good], k=3, ext=3)._eval_args
			assert n[k] == len(t)
			np.testing.assert_array_equal(kn[k, :len(t)], t)
			m = int(good.sum())
			np.testing.assert_allclose(co[k, :m], c[:m], rtol=1e-11, atol=1e-12)


def test_radial_pieces(ctx):
	"""Zero point, ring counts and the spline evaluation, each against numpy / scipy directly."""
	from photometry_amd import prepare
	from scipy.interpolate import InterpolatedUnivariateSpline
	R, C = 320, 384
	f = _tess_frames(1, R, C, seed=9)
	geo = prepare.RadialGeometry((R, C), 1, 1)
	details = {}
	prepare.fit_background_frames(ctx, ctx.array(f), camera=1, ccd=1, bkgiters=1, geometry=geo, details=details)
	mask = ~np.isfinite(f[0]) | (f[0] > 8e4) | (f[0] < 0)
	assert details['zeropoint'][0][0] == -np.float64(f[0][~mask].min()) + 1.0
	counts = np.array([np.sum(~mask.ravel()[geo.ring_pixels[a:b]]) for a, b in zip(geo.ring_offsets[:-1], geo.ring_offsets[1:])])
	assert np.array_equal(details['counts'][0][0], counts)
	# spline evaluation: a known profile through the evaluator, against scipy on the distance image
	x = geo.bin_center
	y = 2.0 + 0.3 * np.sin(x / 100.0)
	y[[3, 4, 17]] = np.nan
	knots, coefs, nk = prepare.radial_profiles(y[None, :], x, radial_smooth=0)
	out = ctx.empty((1, R, C), 'float32')
	zp = ctx.array(np.array([7.5]))
	dk, dc, dn = ctx.array(knots), ctx.array(coefs), ctx.array(nk)
	ctx._check(ctx.lib.tp_radial_evaluate(ctx.handle, 1, R, C, R * C, 44.0, float(geo.xcen), float(geo.ycen), dk.ptr, dc.ptr, dn.ptr, knots.shape[1],
		zp.ptr, None, 0, out.ptr))
	yy, xx = np.mgrid[0:R, 0:C]
	r = np.sqrt((xx + 44 - geo.xcen)**2 + (yy - geo.ycen)**2)
	good = ~np.isnan(y)
	ref = 10**InterpolatedUnivariateSpline(x[good], y[good], k=3, ext=3)(r) - 7.5
	np.testing.assert_allclose(out.to_host()[0], ref, rtol=2e-7, atol=1e-5)


def test_prepare_pixel_flags_and_headers(ctx):
	"""
	prepare_frames with the FFI header cards: manual excludes (pixel_flags.py:13-58: Mars columns, Earth-shine frames, an
	all-zero frame), the background mask as NotUsedForBackground, backgrounds_pixels_used, and the masked pixels staying out
	of the background fit -- against the oracle's restatement of the same lines (rules pinned by golden_pixelflags.npz).
	"""
	from photometry_amd import prepare
	from oracle import backgrounds as ob
	T, R, C = 6, 128, 1600
	rng = np.random.default_rng(11)
	f = (100 + rng.normal(0, 3, (T, R, C))).astype('float32')
	f[0, 3:9, 10:20] = np.nan
	f[1, 20:30, 1540:1550] = 2e5
	f[2, 40, 50] = -1.0
	f[:, 100:110, 200:210] = np.inf              # never usable: backgrounds_pixels_used False there
	f[4] = 0.0                                   # whole image zero
	err = np.ones_like(f)
	headers = {'is_tess': True, 'CAMERA': 1, 'CCD': 4, 'FFIINDEX': [4723, 4724, 4725, 11360, 5000, 5001],
		'TSTART': [1330.0, 1330.02, 1330.04, 1330.06, 1330.08, 1330.10], 'TSTOP': [1330.02, 1330.04, 1330.06, 1330.08, 1330.10, 1330.12]}
	quality = np.zeros(T, dtype='int32')
	first = prepare.manual_exclude_columns(T, C, True, 1, 4, headers['FFIINDEX'], headers['TSTART'], headers['TSTOP'])
	assert list(first) == [1536, 1536, C, 0, C, C]
	flags, allzero = prepare.pixel_flags_frames(ctx, ctx.array(f), first, True)
	assert list(allzero) == [False, False, False, False, True, False]
	manexcl = np.stack([ob.pixel_manual_exclude(f[k], True, 1, 4, headers['FFIINDEX'][k], headers['TSTART'][k], headers['TSTOP'][k]) for k in range(T)])
	masks = np.stack([ob.stamp_mask(f[k], 8e4, manexcl[k]) for k in range(T)])
	ref_flags, ref_used = ob.prepare_pixel_flags(f, masks, manexcl)
	np.testing.assert_array_equal(flags.to_host(), ref_flags)
	assert ref_flags[0, 0, 1536] == 3 and ref_flags[0, 0, 1535] == 0 and np.all(ref_flags[3] == 3) and np.all(ref_flags[4] == 3) and ref_flags[2, 40, 50] == 1

	# the whole stage, flags given (plain background branch)
	res = prepare.prepare_frames(ctx, ctx.array(f), ctx.array(err), quality, pixel_flags=flags)
	np.testing.assert_array_equal(res['backgrounds_pixels_used'].to_host().astype(bool), ref_used)
	assert not ref_used[105, 205] and ref_used[0, 0] and not ref_used[0, 1540]      # columns >= 1536: used in 2 of 6 frames only
	img = res['images'].to_host()
	assert np.all(np.isnan(img[0][:, 1536:])) and np.all(np.isnan(img[3])) and np.all(np.isnan(img[4])) and np.isfinite(img[2, 40, 51])
	# excluded pixels did not take part in the background: frame 1's bright block sits in excluded columns, frames 3 / 4 have no background
	us = prepare.fit_background_frames(ctx, ctx.array(f), exclude=flags).to_host()
	assert np.all(np.isnan(us[3])) and np.all(np.isnan(us[4]))
	for k in (0, 1, 2, 5):
		ref_bkg, _ = ob.fit_background(f[k], exclude=manexcl[k])
		np.testing.assert_allclose(us[k], ref_bkg, rtol=1e-6)

	# ... and from the header cards (TESS branch: radial component with the excluded columns masked)
	res_h = prepare.prepare_frames(ctx, ctx.array(f), ctx.array(err), quality, headers=headers)
	np.testing.assert_array_equal(res_h['pixel_flags'].to_host(), ref_flags)
	np.testing.assert_array_equal(res_h['backgrounds_pixels_used'].to_host().astype(bool), ref_used)
	us_t = prepare.fit_background_frames(ctx, ctx.array(f), exclude=flags, camera=1, ccd=4).to_host()
	for k in (0, 5):
		ref_bkg, _ = ob.fit_background_tess(f[k], 1, 4, exclude=manexcl[k], device_arithmetic=True)
		np.testing.assert_allclose(us_t[k], ref_bkg, rtol=2e-6)
		ref_lit, _ = ob.fit_background_tess(f[k], 1, 4, exclude=manexcl[k])
		# literal float32 log10 of numpy: a ring whose KDE argmax sits on a tie may land on the neighbouring grid point; measured on 32
		# full frames (profiles/r6_tess_flip_stats.txt): 1.3e-4 at worst with a flipped ring, asserted at 5e-4 like the tests above
		np.testing.assert_allclose(us_t[k], ref_lit, rtol=5e-4)
	smooth = np.moveaxis(ob.smooth_time(np.moveaxis(us_t, 0, -1), 3), -1, 0)
	np.testing.assert_array_equal(res_h['backgrounds'].to_host(), smooth)


def test_tess_branch_implicit_images_equal_stored_images(ctx):
	"""fit_background's TESS branch with the radial and the square component evaluated where they are read (tp_background_mesh_radial,
	tp_radial_zeropoint_zoom, tp_radial_ring_modes_zoom, tp_radial_evaluate_zoom: the default) against the same alternation with both
	images stored and re-read (round 4): ring modes, zero points, knots and the background bit for bit -- frames with a manual
	exclusion, a frame that is no multiple of the box size, a frame without a radial component."""
	from photometry_amd import prepare
	for (T, R, C, cam, ccd, excl) in ((2, 512, 512, 1, 1, False), (2, 300, 421, 1, 1, True), (1, 2048, 2048, 3, 2, False)):
		f = _tess_frames(T, R, C, seed=R + C)
		exclude = None
		if excl:
			ex = np.zeros((T, R, C), dtype='uint8')
			ex[:, :, C - 37:] = 1
			ex[1, 100:140, 50:90] = 1
			exclude = ctx.array(ex)
		d_f = ctx.array(f)
		da, db = {}, {}
		a = prepare.fit_background_frames(ctx, d_f, camera=cam, ccd=ccd, exclude=exclude, details=da, implicit=True).to_host()
		b = prepare.fit_background_frames(ctx, d_f, camera=cam, ccd=ccd, exclude=exclude, details=db, implicit=False).to_host()
		for key in ('s2', 'zeropoint', 'n_knots', 'counts'):
			for it in range(3):
				np.testing.assert_array_equal(da[key][it], db[key][it], err_msg=f'{key} round {it} of a {R} x {C} frame')
		np.testing.assert_array_equal(a, b)
		assert np.isfinite(a).all()

def test_mesh_path_hand_cases_on_device(ctx):
	"""The hand-derived cases of tests/test_oracle_pins.py (photutils Background2D after the cell statistics) through the device
	entries: tp_background_mesh_finish (IDW fill of a rejected cell from its ten nearest kept cells, 2048 / 2049 masked pixels,
	fewer kept cells than neighbours, the NaN-ignoring 3 x 3 median at corners and edges), tp_background_zoom (3 x 3 ramp mesh
	against the hand formula, a 32 x 32 mesh against the tridiagonal solve, frame edges and cropped last cells) and the whole
	fit_background_frames on a frame that is no multiple of 64 and on one where only the SECOND mesh selection (after the
	sigma clip) rejects a cell."""
	import test_oracle_pins as pins
	from photometry_amd import prepare

	def finish(mesh, nm, filter_size):
		ny, nx = mesh.shape
		d_mesh, d_nm = ctx.array(np.ascontiguousarray(mesh[None], dtype='float64')), ctx.array(np.ascontiguousarray(nm[None], dtype='int32'))
		coef, vmin, vmax, filt = ctx.empty((1, ny, nx), 'float64'), ctx.empty((1,), 'float64'), ctx.empty((1,), 'float64'), ctx.empty((1, ny, nx), 'float64')
		ctx._check(ctx.lib.tp_background_mesh_finish(ctx.handle, d_mesh.ptr, d_nm.ptr, 1, ny, nx, 64, 50.0, filter_size, coef.ptr, vmin.ptr, vmax.ptr, filt.ptr))
		return filt.to_host()[0], coef, vmin, vmax

	mesh, nm, expect = pins.mesh_idw_case()
	got = finish(mesh, nm, 1)[0]
	assert abs(got[2, 2] - expect) < 1e-13 * expect
	keep = np.ones((5, 5), bool); keep[2, 2] = False
	np.testing.assert_array_equal(got[keep], mesh[keep])
	mesh, nm, expect = pins.mesh_few_cells_case()
	got = finish(mesh, nm, 1)[0]
	assert abs(got[0, 0] - expect) < 1e-14 * expect and got[0, 1] == 4.0 and got[1, 0] == 8.0 and got[1, 1] == 16.0
	np.testing.assert_array_equal(finish(pins.MEDIAN_3X3_IN, np.zeros((3, 3), dtype='int32'), 3)[0], pins.MEDIAN_3X3_OUT)
	assert np.all(np.isnan(finish(np.ones((2, 2)), np.full((2, 2), 4096, dtype='int32'), 3)[0]))   # nothing kept: NaN (photutils raises)

	def zoom(mesh, box, R, C):
		ny, nx = mesh.shape
		_, coef, vmin, vmax = finish(mesh, np.zeros(mesh.shape, dtype='int32'), 1)
		out = ctx.empty((1, R, C), 'float32')
		ctx._check(ctx.lib.tp_background_zoom(ctx.handle, coef.ptr, vmin.ptr, vmax.ptr, 1, ny, nx, box, R, C, C, R * C, out.ptr))
		return out.to_host()[0].astype('float64')

	ramp = 10.0 + np.arange(3)[None, :] + 3.0 * np.arange(3)[:, None]
	for box, (R, C) in ((64, (192, 192)), (64, (150, 131)), (4, (12, 12))):
		got = zoom(ramp, box, R, C)
		# the hand answer within scipy's three-sample prefilter deviation (see test_zoom_of_a_ramp_mesh_by_hand) ...
		np.testing.assert_allclose(got, pins.zoom_ramp_expected(box, R, C), rtol=0, atol=5e-3)
		assert got[0, 0] == 10.0 and ((R, C) == (150, 131) or got[-1, -1] == 18.0)   # the spline overshoots the corners: clipped to the mesh range
	m32 = pins.zoom_mesh_32()
	want = pins.exact_zoom(m32, 4)
	# ... and exactly (float32 output: 6e-8 relative) where the mesh has the size of a real frame's
	np.testing.assert_allclose(zoom(m32, 4, 128, 128), want, rtol=1.2e-7)
	np.testing.assert_allclose(zoom(m32, 4, 126, 125), want[:126, :125], rtol=1.2e-7)

	# a single row / column of cells: the 1-D case (scipy leaves an axis of length one alone, the zoom is constant along it)
	from scipy import ndimage
	for shape in ((1, 5), (4, 1), (1, 1)):
		m1 = np.random.default_rng(3).normal(50, 3, shape)
		want1 = np.clip(ndimage.zoom(m1, 8, order=3, mode='reflect', grid_mode=True), m1.min(), m1.max())
		np.testing.assert_allclose(zoom(m1, 8, 8 * shape[0], 8 * shape[1]), want1, rtol=1.2e-7)

	img, expect = pins.make_ragged_frame()
	bkg, mesh, nmasked = prepare.fit_background_frames(ctx, ctx.array(img[None]), return_mask=True)
	np.testing.assert_array_equal(nmasked[0], [[0, 3712], [1792, 3880]])
	np.testing.assert_array_equal(mesh[0], [[5.0, 1234.0], [9.0, 0.5]])
	np.testing.assert_allclose(bkg.to_host()[0], expect, rtol=1e-7)
	img, expect = pins.make_second_selection_frame()
	bkg, mesh, nmasked = prepare.fit_background_frames(ctx, ctx.array(img[None]), return_mask=True)
	np.testing.assert_array_equal(nmasked[0].ravel(), [2050, 0])          # 2040 masked + the 10 pixels the sigma clip rejected
	np.testing.assert_array_equal(mesh[0].ravel(), [100.0, 300.0])
	np.testing.assert_allclose(bkg.to_host()[0], expect, rtol=1e-7)


def test_median_filter_15_shared_columns(ctx):
	"""The 15 x 15 median filter, four output pixels per sort of their shared columns: frames wider than one workgroup's 128
	columns with a ragged last block, image edges (reflection) on all sides, runs of +inf / NaN / -inf pixels -- scipy on the
	same values is the check (non-finite -> +inf, which sorts last; a window whose median is non-finite gives NaN)."""
	from scipy.ndimage import median_filter
	rng = np.random.default_rng(21)
	for (R, C, with_ref) in ((37, 301, True), (15, 15, False), (16, 128, False), (64, 129, True)):
		img = rng.normal(0, 3, (2, R, C)).astype('float32')
		img[0, R // 2:, : C // 3] = rng.integers(-2, 3, (R - R // 2, C // 3)).astype('float32')   # many equal values
		bad = rng.random((2, R, C)) < 0.02
		img[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype='float32'), int(bad.sum()))
		img[1, 3:14, 5:14] = np.nan                                   # a hole larger than half a window
		ref = rng.normal(0, 1, (R, C)) if with_ref else None
		out = ctx.empty((2, R, C), 'float32')
		d_img = ctx.array(img)                       # (kept alive: a temporary's block goes back to the allocation cache at once)
		d_ref = ctx.array(ref) if with_ref else None
		ctx._check(ctx.lib.tp_frames_median_filter(ctx.handle, d_img.ptr, 2, R, C, C, R * C, d_ref.ptr if with_ref else None, 15, out.ptr))
		got = out.to_host()
		for k in range(2):
			x = (img[k].astype('float64') - ref).astype('float32') if with_ref else img[k].copy()
			x[~np.isfinite(x)] = np.inf
			want = median_filter(x, size=15)
			want[~np.isfinite(want)] = np.nan
			np.testing.assert_array_equal(got[k], want)


# ---- the ring kernel and the profile kernel at their own boundaries (hand-made rings: the camera geometry never gives these) ----------
HAND_RING_SIZES = (0, 1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097)
HAND_CUTOFF = 8e4


def _hand_rings(seed=3):
	"""Two 64 x 80 frames and 19 hand-made rings over them (rings share pixels): lists of the sizes around the ring kernel's block (256)
	and batch (2048) boundaries, each sprinkled with masked pixels of the four kinds (negative, above the cutoff, NaN, manually
	excluded) so that the ordered compaction matters; three rings whose KEPT count sits on 256 / 2048 / 2049; an all-equal ring of odd
	and one of even kept count (zero bandwidth: the median -- 3 and 8 samples, whose sum and mean are exact in every order
	of summation, so that neither side's standard deviation is a rounding residue); a ring of kept count 0 and one of kept count 1 after masking.  The second
	frame has further NaN pixels, so its kept counts differ.  The kept pixels' logarithms are ``2.0 + normal(0, 2e-3)`` to float32
	rounding (the samples of test_radial_rules_host).  Returns a dict: ``frames`` (2, 64, 80) float32, ``exclude`` (64, 80) uint8,
	``square`` (2, 64, 80) float32 (constant on the all-equal rings), ``pixels`` / ``offsets`` int32, ``names``."""
	rng = np.random.default_rng(seed)
	R, C = 64, 80
	P = R * C
	perm = rng.permutation(P)
	masked, equal, small, big, zero = perm[:400], perm[400:440], perm[440:520], perm[520:-1], perm[-1]
	f = np.empty((2, P), dtype='float32')
	for k in range(2):
		f[k] = (10.0**(2.0 + rng.normal(0, 2e-3, P)) - 1.0).astype('float32')
	f[:, masked[:100]] = -3.0
	f[:, masked[100:200]] = 9e4
	f[:, masked[200:300]] = np.nan
	exclude = np.zeros(P, dtype='uint8')
	exclude[masked[300:400]] = 1
	f[:, equal] = 150.0
	f[:, zero] = 0.0                                                    # the frames' minimum, in no ring: zero point 1
	f[1, big[rng.random(len(big)) < 0.03]] = np.nan                       # frame 1 only: other kept counts in the large rings
	square = (20.0 + 0.05 * np.arange(P) / C + rng.normal(0, 0.01, (2, P))).astype('float32')
	square[:, equal] = 20.0

	def sprinkled(good, n_masked):
		"""``good`` with ``n_masked`` masked pixels at random places of the list"""
		ring = np.concatenate([good, rng.choice(masked, n_masked, replace=False)])
		where = rng.permutation(len(ring))
		return ring[where]
	rings, names = [], []
	for S in HAND_RING_SIZES:
		nm = min(S // 10, 300) if S > 3 else 0
		rings.append(sprinkled(rng.choice(big if S > 3 else small, S - nm, replace=False), nm)); names.append(f'list of {S}')
	for S in (256, 2048, 2049):
		rings.append(sprinkled(rng.choice(big, S, replace=False), 31)); names.append(f'{S} kept in frame 0')
		assert np.isnan(f[0, rings[-1]]).sum() == np.isin(rings[-1], masked[200:300]).sum()     # frame 0: no NaN but the sprinkled ones
	rings.append(sprinkled(equal[:3], 3)); names.append('all equal, 3 kept')
	rings.append(sprinkled(equal[3:11], 2)); names.append('all equal, 8 kept')
	rings.append(masked[[0, 100, 200, 300, 1]].copy()); names.append('0 kept')
	rings.append(np.array([masked[2], masked[101], small[0], masked[201], masked[301]])); names.append('1 kept')
	rings.append(np.array([masked[3], small[1], masked[102], small[2]])); names.append('2 kept')
	offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype('int32')
	return {'frames': f.reshape(2, R, C), 'exclude': exclude.reshape(R, C), 'square': square.reshape(2, R, C),
		'pixels': np.concatenate(rings).astype('int32'), 'offsets': offsets, 'names': names}


def _hand_ring_logs(h, with_square):
	"""Per frame the zero point and per ring the kept pixels' logarithms, in list order, as ``fit_background_tess(device_arithmetic=True)``
	forms them: first round float32 arithmetic with the correctly rounded float32 log10, with a square component float64."""
	from oracle import backgrounds as ob
	zps, logs = [], []
	for k in range(2):
		img = h['frames'][k].ravel()
		keep = ~ob.stamp_mask(img, HAND_CUTOFF, h['exclude'].ravel())
		if with_square:
			v = img.astype('float64') - h['square'][k].ravel().astype('float64')
			zp = -np.min(v[keep]) + 1.0
			arg = np.where(keep, v, 1.0) + zp
		else:
			zp = -np.float64(np.min(img[keep])) + 1.0
			arg = (np.where(keep, img, np.float32(1)) + np.float32(zp)).astype('float64')
		u, inverse = np.unique(arg, return_inverse=True)                  # (one log10 per value: numpy's vector and scalar loops differ by an ulp)
		lg = np.log10(u)[inverse]
		if not with_square:
			lg = lg.astype('float32').astype('float64')
		zps.append(zp)
		logs.append([lg[p][keep[p]] for p in (h['pixels'][a:b] for a, b in zip(h['offsets'][:-1], h['offsets'][1:]))])
	return np.array(zps), logs


def _run_hand_rings(ctx, h, with_square):
	zps, logs = _hand_ring_logs(h, with_square)
	n_rings, P = len(h['offsets']) - 1, h['frames'][0].size
	d_f, d_ex, d_sq, d_zp = ctx.array(h['frames']), ctx.array(h['exclude']), ctx.array(h['square']), ctx.array(zps)
	d_pix, d_off = ctx.array(h['pixels']), ctx.array(h['offsets'])
	out = []
	for _ in range(2):
		scratch, modes, counts = ctx.empty((2, int(h['offsets'][-1])), 'float64'), ctx.empty((2, n_rings), 'float64'), ctx.empty((2, n_rings), 'int32')
		ctx._check(ctx.lib.tp_radial_ring_modes(ctx.handle, d_f.ptr, 2, P, P, d_sq.ptr if with_square else None, P, d_ex.ptr, 0, HAND_CUTOFF, d_zp.ptr,
			d_pix.ptr, d_off.ptr, n_rings, int(h['offsets'][-1]), float(radial_common.BW_CONSTANT), scratch.ptr, modes.ptr, counts.ptr))
		out.append((modes.to_host(), counts.to_host()))
	return zps, logs, out


@pytest.mark.parametrize('with_square', (False, True))
def test_ring_modes_of_hand_made_rings(ctx, with_square):
	"""tp_radial_ring_modes called directly with the rings of ``_hand_rings``, two frames in one call, without a square image (float32
	first-round arithmetic) and with one (float64): the counts exact, the modes against ``oracle.backgrounds.reduce_mode(binning='fixed')``
	on the logarithms of the kept pixels in list order -- same NaN pattern, same grid point (radial_common: what that is held to and
	the margin asserted on the oracle), the all-equal rings exactly their value -- and a second call bit for bit the same."""
	import warnings
	h = _hand_rings()
	zps, logs, ((modes, counts), (modes2, counts2)) = _run_hand_rings(ctx, h, with_square)
	assert np.array_equal(modes.view('uint64'), modes2.view('uint64')) and np.array_equal(counts, counts2)
	assert np.array_equal(counts, [[len(x) for x in frame] for frame in logs])
	assert list(counts[0][:4]) == [0, 1, 2, 3] and list(counts[0][11:14]) == [256, 2048, 2049] and list(counts[0][14:]) == [3, 8, 0, 1, 2]
	assert counts[0][10] > 2048 + 1024 and np.all(counts[1][4:14] <= counts[0][4:14]) and np.any(counts[1][4:14] < counts[0][4:14])
	rules = []
	for k in range(2):
		for j, x in enumerate(logs[k]):
			with warnings.catch_warnings():
				warnings.simplefilter('ignore', RuntimeWarning)
				rules.append(radial_common.assert_same_mode(modes[k, j], x, label=(k, h['names'][j])))
	per_frame = ['nan', 'nan', 'tie'] + ['argmax'] * 11 + ['median', 'median', 'nan', 'nan', 'tie']
	assert rules == per_frame * 2
	for k in range(2):
		assert modes[k, 14] == logs[k][14][0] and modes[k, 15] == logs[k][15][0]


def test_ring_profiles_of_64_rings_and_of_exactly_four(ctx):
	"""tp_radial_profiles at the kernel's limit of 64 rings (68 knots: the lanes take two turns at the knots) and with exactly 4
	usable rings (the smallest system; 3 give none), with the assertions of test_mesh_finish_and_ring_profiles_on_device."""
	from scipy.interpolate import InterpolatedUnivariateSpline
	from photometry_amd import prepare
	rng = np.random.default_rng(22)
	nr = 64
	bc = 2400.0 + 15.0 * np.arange(nr) + 7.5
	s2 = 2.0 + 0.3 * np.sin(bc / 100.0)[None, :] + rng.normal(0, 2e-3, (5, nr))
	s2[1, [0, 1, 30, 31, 32, 63]] = np.nan
	s2[2, :] = np.nan; s2[2, [2, 9, 40, 63]] = [2.0, 2.2, 2.1, 2.4]         # exactly 4 usable rings
	s2[3, :] = np.nan; s2[3, [2, 40, 63]] = [2.0, 2.1, 2.4]                 # 3: no spline
	s2[4, ::2] = np.nan
	seen = set()
	for smooth in (0, 3, 8):
		K = nr + 4
		knots, coefs, nk = ctx.zeros((5, K), 'float64'), ctx.zeros((5, K), 'float64'), ctx.zeros((5,), 'int32')
		d_s2, d_bc = ctx.array(s2), ctx.array(bc)
		ctx._check(ctx.lib.tp_radial_profiles(ctx.handle, 5, nr, d_s2.ptr, d_bc.ptr, smooth, K, knots.ptr, coefs.ptr, nk.ptr))
		kn, co, n = knots.to_host(), coefs.to_host(), nk.to_host()
		for k in range(5):
			prof = prepare._move_median_central(s2[k], smooth) if smooth else s2[k]
			good = ~np.isnan(prof)
			seen.add(int(good.sum()))
			if good.sum() < 4:
				assert n[k] == 0
				continue
			t, c, _ = InterpolatedUnivariateSpline(bc[good], prof[good], k=3, ext=3)._eval_args
			assert n[k] == len(t)
			np.testing.assert_array_equal(kn[k, :len(t)], t)
			m = int(good.sum())
			np.testing.assert_allclose(co[k, :m], c[:m], rtol=1e-11, atol=1e-12)
	assert {64, 4, 3} <= seen
