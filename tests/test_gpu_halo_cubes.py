# -*- coding: utf-8 -*-
"""
The cubes path of Halo photometry (csrc/halo_cubes.hip: ``tp_halo_select_cubes``, ``tp_halo_gather_cubes``, ``tp_halo_outputs_cubes``)
through the C ABI and through ``halo.photometry_cubes``, against the host restatement ``halo.build_problems`` / ``halo.pack`` /
``halo.photometry``: pixels, cadences, fit flags, counts and ``P`` bit for bit; median, ``corr_flux``, ``flux`` and the weight maps
bit for bit; ``flux_err`` within the bound of tests/test_gpu_halo_frames.py (the device sums the stamp's pixels in ascending order,
numpy's nansum pairwise: up to 4 096 non-negative float64 terms in two orders).
"""
import numpy as np
import pytest
import halo_cubes_common as cc

pytestmark = pytest.mark.gpu

#: the last two are the stamp limit: 45 x 46 = 2070 pixels (more than 2048 kept: float4 column 2 of the solver's backward kernel) and
#: 64 x 64 = 4096, the largest stamp the entries take
SHAPES = ((1, 1, 3), (3, 5, 63), (3, 5, 64), (3, 5, 65), (9, 13, 70), (11, 11, 130), (45, 46, 65), (64, 64, 70))
LIMIT_SHAPES = SHAPES[-2:]
PADS = (np.nan, 1e30)
FLUX_ERR_RTOL = 4096 * 2.0**-53
MINFLUX = -100.0


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _targets(shape, n_segs, seed):
	"""``len(n_segs)`` targets of one shape, each with its own NaN / inf cadences, pixels below and around ``minflux``, quality row and
	segments (``n_segs[i]`` of them, and a few cadences without one)."""
	H, W, T = shape
	n = len(n_segs)
	rng = np.random.default_rng(seed)
	images = rng.uniform(50, 1000, (n, H, W, T)).astype('float32')
	masks = np.ones((n, H, W), dtype=bool)
	if H * W > 1:
		# (a cadence is lost with one bad value in any kept pixel: a large stamp gets fewer of them, so that about a quarter is lost)
		for value in (np.nan, np.inf, -np.inf):
			images[rng.random(images.shape) < (0.002 if H * W <= 2048 else 0.1 / (H * W))] = value
		flat = images.reshape(n, H * W, T)
		flat[:, 1, :] = (-500.0 + rng.normal(size=(n, T))).astype('float32')                 # far below minflux: dropped
		flat[:, 2, :] = (-100.0 + rng.normal(size=(n, T))).astype('float32')                 # scattered round minflux: by the median
		flat[:, 3, : T // 2] = -300.0                                                        # below in the first half only
		masks = rng.random((n, H, W)) < (0.85 if H * W <= 2048 else 0.995)   # (a large stamp keeps more than 2048 pixels)
		masks.reshape(n, -1)[:, :5] = True
	quality = np.where(rng.random((n, T)) < 0.1, 32, 0).astype('int32')
	segs = np.zeros((n, T), dtype='int64')
	for i, k in enumerate(n_segs):
		segs[i] = np.minimum(np.arange(T) * k // T, k - 1)
		if T > 8:
			segs[i, rng.choice(T - 1, size=2, replace=False)] = -1
			segs[i, -1] = k - 1
	return images, masks, quality, segs


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_tile_and_wave_edges(ctx, shape):
	"""One and two segments side by side at the sizes round the wavefront (63, 64, 65 cadences), the tile of the transposition and
	the smallest cube; the pads behind the last cadence hold NaN in one run and 1e30 in the other: the results are the same."""
	images, masks, quality, segs = _targets(shape, (1, 2) if shape[2] > 3 else (1, 1), seed=sum(shape))
	runs = []
	for pad in PADS:
		cube = cc.device_cube(ctx, images, pad)
		dev, cadpos = cc.select_gather(ctx, cube, masks, segs, quality)
		cube.free()
		cc.hold_problems(dev, cadpos, images, masks, segs, quality, f'{shape} pad {pad}')
		runs.append((dev, cadpos))
	(a, pos_a), (b, pos_b) = runs
	assert np.array_equal(pos_a, pos_b)
	for pa, pb in zip(a, b):
		for x, y in zip(pa, pb):
			assert all(np.array_equal(x[key], y[key]) for key in ('pix', 'cad', 'fit'))
			assert cc.same_bits(x['P'], y['P'])
	if shape[0] * shape[1] > 1:
		assert any(len(p['pix']) < masks[i].sum() for i, per in enumerate(a) for p in per), 'no pixel was dropped: the case shows nothing'
		assert any(len(p['cad']) < np.count_nonzero(segs[i] == k) for i, per in enumerate(a) for k, p in enumerate(per))
	if shape in LIMIT_SHAPES:
		assert any(len(p['pix']) > 2048 for per in a for p in per), [len(p['pix']) for per in a for p in per]


def test_mixed_segment_counts(ctx):
	"""Targets with one, two and three segments in one group, each with its own quality row and NaN cadences."""
	images, masks, quality, segs = _targets((5, 7, 100), (1, 2, 3, 2, 1), seed=5)
	cube = cc.device_cube(ctx, images, np.nan)
	dev, cadpos = cc.select_gather(ctx, cube, masks, segs, quality)
	cube.free()
	assert [len(per) for per in dev] == [1, 2, 3, 2, 1]
	cc.hold_problems(dev, cadpos, images, masks, segs, quality, 'mixed')
	assert not np.array_equal(quality[0], quality[1]) and not np.array_equal(dev[1][0]['cad'], dev[3][0]['cad'])


def _gap_times(T):
	"""Cadences 0.03 d apart with a gap of 0.54 d before cadence ``T // 2``: the gap rule of the split times finds it (the cadence before
	it lies between 30 % and 70 % of the span for 12 <= T), so cadences ``T // 2`` and later are segment 1."""
	regular = 1500.0 + np.arange(T) * 0.03
	return np.where(np.arange(T) < T // 2, regular, regular + 0.51)


def _edge_targets():
	"""Four targets of 4 x 5 x 40: 0 has a segment without a cadence (1 of 0 .. 2), 1 has two fitted cadences in its second segment,
	2 loses every pixel of its first segment, 3 is ordinary."""
	images, masks, quality, segs = _targets((4, 5, 40), (3, 2, 2, 2), seed=9)
	segs[0] = np.where(np.arange(40) < 20, 0, 2)
	quality[1] = 0
	quality[1, 20:38] = 32
	segs[1] = np.arange(40) >= 20
	images[1][np.isnan(images[1]) | np.isinf(images[1])] = 200.0
	segs[2] = np.arange(40) >= 20
	images[2][:, :, :20] = -500.0
	segs[3] = np.arange(40) >= 20
	times = np.stack([np.linspace(1346.5, 1350.0, 40), _gap_times(40), _gap_times(40), _gap_times(40)])
	times[0, 20:] = np.linspace(1349.4, 1350.0, 20)
	times[0, :20] = np.linspace(1346.5, 1347.3, 20)                                         # nothing in (1347.366, 1349.315)
	return images, masks, quality, segs, times, np.array([1, -1, -1, -1])


def test_segment_edge_cases(ctx):
	from photometry_amd import halo
	images, masks, quality, segs, times, sector = _edge_targets()
	n, T = 4, 40
	cube = cc.device_cube(ctx, images, np.nan)
	dev, cadpos = cc.select_gather(ctx, cube, masks, segs, quality)
	cc.hold_problems(dev, cadpos, images, masks, segs, quality, 'edge cases')
	# a segment without a cadence keeps every mask pixel
	np.testing.assert_array_equal(dev[0][1]['pix'], np.flatnonzero(masks[0].ravel()))
	assert len(dev[0][1]['cad']) == 0
	# every pixel of segment 0 of target 2 is dropped: nothing of the target is packed
	assert len(dev[2][0]['pix']) == 0 and dev[2][0]['P'] is None and dev[2][1]['P'] is None and len(dev[2][1]['pix']) > 0
	err = cc.device_cube(ctx, np.ones_like(images), np.nan)
	args = (masks, times, np.zeros((n, T)), np.tile(np.arange(T), (n, 1)), quality, sector, np.full(n, 1000.0))
	res = halo.photometry_cubes(ctx, {'images': cube, 'images_err': err}, *args)
	for i in range(n):
		np.testing.assert_array_equal(res['segments'][i], segs[i])
	assert list(res['usable']) == [True, True, False, True]
	assert res['status'][0][1] == halo.DEGENERATE                                           # no cadence at all
	assert int(np.sum(dev[1][1]['fit'])) == 2 and res['status'][1][1] == halo.DEGENERATE and res['status'][1][0] != halo.DEGENERATE
	assert np.all(np.isnan(res['corr_flux'][1][segs[1] == 1])) and np.all(np.isfinite(res['corr_flux'][1][dev[1][0]['cad']]))
	assert res['weightmap'][2] is None and np.all(np.isnan(res['corr_flux'][2])) and not res['flux_err'][2].any()
	assert res['status'][3][0] != halo.DEGENERATE and res['status'][3][1] != halo.DEGENERATE
	# the neighbours of the degenerate and the unusable target are what they are alone
	for i in (0, 3):
		one = halo.photometry_cubes(ctx, {'images': cube.slice0(i, 1), 'images_err': err.slice0(i, 1)}, *(a[i:i + 1] for a in args))
		_same_target(one, 0, res, i)
	cube.free()
	err.free()


def test_the_minflux_decision_at_its_edges(ctx):
	"""numpy's ``nanmedian(float64) < minflux`` on the pixels that sit on the decision: 8 fitted cadences and 2 that are not."""
	T = 10
	images = np.full((1, 1, 5, T), 300.0, dtype='float32')
	quality = np.zeros((1, T), dtype='int32')
	quality[0, [3, 7]] = 32
	fitted = np.flatnonzero(quality[0] == 0)
	px = images[0, 0]
	px[0, fitted] = -200.0                                                                  # constant below: dropped
	px[0, [3, 7]] = 1e6                                                                     # (what is not fitted does not count)
	px[1, fitted[::2]], px[1, fitted[1::2]] = -150.0, -50.0                                 # median exactly -100: kept
	px[2, fitted[::2]], px[2, fitted[1::2]] = -150.0, np.nextafter(np.float32(-50.0), np.float32(-np.inf))   # one ulp lower: dropped
	px[3, fitted] = np.nan                                                                  # NaN at every fitted cadence: kept
	masks = np.ones((1, 1, 5), dtype=bool)
	segs = np.zeros((1, T), dtype='int64')
	med = np.array([np.nanmedian(px[p, fitted].astype('float64')) if p != 3 else np.nan for p in range(5)])
	assert med[1] == MINFLUX and med[2] < MINFLUX and med[2] > MINFLUX - 1e-5
	cube = cc.device_cube(ctx, images, np.nan)
	dev, cadpos = cc.select_gather(ctx, cube, masks, segs, quality)
	cube.free()
	np.testing.assert_array_equal(dev[0][0]['pix'], [1, 3, 4])
	np.testing.assert_array_equal(dev[0][0]['pix'], np.flatnonzero(~(med < MINFLUX)))
	np.testing.assert_array_equal(dev[0][0]['cad'], [3, 7])                                 # pixel 3 is finite where it was not fitted
	cc.hold_problems(dev, cadpos, images, masks, segs, quality, 'minflux edges')


def test_the_cadence_rule(ctx):
	"""A kept pixel's inf and NaN remove their cadences; a dropped pixel's NaN removes nothing."""
	T = 20
	images = np.full((1, 2, 3, T), 500.0, dtype='float32')
	images[0, 0, 0, 4], images[0, 0, 0, 9] = np.inf, np.nan
	images[0, 1, 1, :] = -500.0
	images[0, 1, 1, 12] = np.nan
	masks, segs, quality = np.ones((1, 2, 3), dtype=bool), np.zeros((1, T), dtype='int64'), np.zeros((1, T), dtype='int32')
	cube = cc.device_cube(ctx, images, 1e30)
	dev, cadpos = cc.select_gather(ctx, cube, masks, segs, quality)
	cube.free()
	np.testing.assert_array_equal(dev[0][0]['pix'], [0, 1, 2, 3, 5])
	np.testing.assert_array_equal(dev[0][0]['cad'], [t for t in range(T) if t not in (4, 9)])
	cc.hold_problems(dev, cadpos, images, masks, segs, quality, 'cadence rule')


# ---- outputs ----------------------------------------------------------------------------------------------------------------------
def _group(shape, seed):
	"""Three targets with one, two and three segments from their own time rows: a regular axis, one with a gap of 0.6 d (the gap
	rule) and one of sector 1 (two of the table's split times inside).  Returns the arguments of ``photometry_cubes`` after the cubes."""
	H, W, T = shape
	images, masks, quality, _ = _targets(shape, (1, 1, 1), seed)
	rng = np.random.default_rng(seed + 1)
	errs = rng.uniform(1, 30, images.shape).astype('float32')
	errs[rng.random(errs.shape) < 0.003] = np.nan
	times = np.stack([1500.0 + np.arange(T) * 0.03, _gap_times(T), np.linspace(1345.0, 1350.0, T)])
	times[0, 7] = np.nan                                                                    # a cadence without a time: no segment
	timecorr = rng.normal(3e-3, 1e-5, (3, T))
	cadenceno = 1000 + np.tile(np.arange(T), (3, 1))
	return images, errs, (masks, times, timecorr, cadenceno, quality, np.array([-1, -1, 1]), np.array([1000.0, -2.5e5, 7.25e4]))


def _same_target(a, i, b, j):
	for name in ('corr_flux', 'flux', 'flux_err'):
		assert cc.same_bits(a[name][i], b[name][j]), name
	assert a['usable'][i] == b['usable'][j]
	for name in ('f', 'iterations', 'status', 'npix', 'ncad', 'median'):
		assert cc.same_bits(a[name][i], b[name][j]), name
	for name in ('w', 'weightmap'):
		assert (a[name][i] is None) == (b[name][j] is None)
		if a[name][i] is not None:
			assert len(a[name][i]) == len(b[name][j]) and all(cc.same_bits(x, y) for x, y in zip(a[name][i], b[name][j])), name


def _hold_outputs(ctx, res, images, errs, args, label):
	from photometry_amd import halo
	masks, times, timecorr, cadenceno, quality, sector, normfactor = args
	worst = 0.0
	for i in range(len(images)):
		ref = halo.photometry(ctx, images[i], errs[i], quality[i], times[i], timecorr[i], cadenceno[i], masks[i], sector[i], normfactor[i])
		where = f'{label} target {i}'
		assert res['usable'][i] and res['split_times'][i] == ref['split_times'], where
		np.testing.assert_array_equal(res['segments'][i], ref['segments'])
		assert len(ref['w']) == len(res['w'][i]) == int(ref['segments'].max()) + 1
		assert cc.same_bits(res['corr_flux'][i], ref['corr_flux']) and cc.same_bits(res['flux'][i], ref['flux']), where
		assert cc.same_bits(res['f'][i], ref['f']) and np.array_equal(res['iterations'][i], ref['iterations']) and np.array_equal(res['status'][i], ref['status']), where
		assert res['initial_cadence'][i] == ref['weightmap']['initial_cadence'] and res['final_cadence'][i] == ref['weightmap']['final_cadence']
		# numpy's median of the segment's light curve over its fitted cadences, from the solver's own l
		probs = halo.build_problems(images[i], quality[i], masks[i], ref['segments'])
		sol = halo.tvmin(ctx, probs)
		for k, p in enumerate(probs):
			assert cc.same_bits(res['w'][i][k], ref['w'][k]) and cc.same_bits(res['weightmap'][i][k], ref['weightmap']['weightmap'][k]), (where, k)
			assert cc.same_bits(np.float64(res['median'][i][k]), np.float64(np.median(sol['l'][k][np.asarray(p.fit, dtype=bool)]))), (where, k)
		err = np.abs(res['flux_err'][i] - ref['flux_err'])
		assert np.all(err <= FLUX_ERR_RTOL * np.abs(ref['flux_err'])), (where, float(np.max(err / np.where(ref['flux_err'] > 0, ref['flux_err'], 1.0))))
		assert np.all(res['flux_err'][i][ref['segments'] < 0] == 0.0) and np.any(ref['flux_err'] > 0)
		worst = max(worst, float(np.max(err / np.where(ref['flux_err'] > 0, ref['flux_err'], 1.0))))
	print(f"{label}: worst relative flux_err difference {worst:.3e} (bound {FLUX_ERR_RTOL:.3e})")


@pytest.mark.parametrize('shape', ((3, 5, 65), (9, 13, 70)) + LIMIT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_outputs_equal_the_per_target_path(ctx, shape):
	from photometry_amd import halo
	images, errs, args = _group(shape, seed=17 + shape[2])
	runs = []
	for pad in PADS:
		cubes = {'images': cc.device_cube(ctx, images, pad), 'images_err': cc.device_cube(ctx, errs, pad)}
		runs.append(halo.photometry_cubes(ctx, cubes, *args))
		for c in cubes.values():
			c.free()
	assert [len(s) for s in runs[0]['status']] == [1, 2, 3]
	_hold_outputs(ctx, runs[0], images, errs, args, f'{shape}')
	for i in range(3):
		_same_target(runs[1], i, runs[0], i)


def test_batch_independence(ctx):
	"""A target gives the same bits inside the group, alone in cubes of its own, as a chosen slot, and with a budget that forces one
	target per chunk."""
	from photometry_amd import halo
	images, errs, args = _group((9, 13, 70), seed=3)
	cubes = {'images': cc.device_cube(ctx, images, np.nan), 'images_err': cc.device_cube(ctx, errs, np.nan)}
	whole = halo.photometry_cubes(ctx, cubes, *args)
	ctx.profile(True)
	ctx.profile_reset()
	chunked = halo.photometry_cubes(ctx, cubes, *args, budget_bytes=1)
	ctx.sync()
	report = ctx.profile_report()
	ctx.profile(False)
	assert report['tp_halo_cube_stat_kernel'][0] == 3 and report['tp_halo_cube_gather_kernel'][0] == 3 and report['tp_halo_cube_lightcurve_kernel'][0] == 3, report
	outer = halo.photometry_cubes(ctx, cubes, *args, targets=[0, 2])                       # (slot 1 travels as a problem without pixels)
	assert outer['w'][1] is None and not outer['usable'][1]
	for i in range(3):
		_same_target(chunked, i, whole, i)
		alone = halo.photometry_cubes(ctx, {k: c.slice0(i, 1) for k, c in cubes.items()}, *(a[i:i + 1] for a in args))
		_same_target(alone, 0, whole, i)
		if i != 1:
			_same_target(outer, i, whole, i)
	for c in cubes.values():
		c.free()


# ---- argument checks --------------------------------------------------------------------------------------------------------------
def _select_raises(ctx, match, H=4, W=5, T=8, prob_off=(0, 1, 2), seg=None):
	import ctypes
	from photometry_amd._lib import TessphotError
	n = len(prob_off) - 1
	dummy = ctx.zeros((1 << 16,), 'int32')                                   # (never touched: the checks come before any launch)
	prob_off = np.array(prob_off, dtype='int32')
	seg = np.zeros((n, T), dtype='int32') if seg is None else np.ascontiguousarray(seg, dtype='int32')
	quality = np.zeros((n, T), dtype='int32')
	p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
	ctx.profile(True)
	ctx.profile_reset()
	with pytest.raises(TessphotError, match=match):
		ctx._check(ctx.lib.tp_halo_select_cubes(ctx.handle, dummy.ptr, n, H, W, T, 32, dummy.ptr, p(prob_off), p(seg), p(quality), 175, -100.0, dummy.ptr, dummy.ptr,
			dummy.ptr, dummy.ptr, dummy.ptr, dummy.ptr))
	ctx.sync()
	report = ctx.profile_report()
	ctx.profile(False)
	dummy.free()
	assert not any('halo' in name for name in report), report


def test_argument_checks(ctx):
	_select_raises(ctx, 'a stamp holds 1 .. 4096 pixels', H=65, W=64)
	_select_raises(ctx, '1 .. 64 segments per target', prob_off=(0, 65, 66))
	bad = np.zeros((2, 8), dtype='int32')
	bad[1, 3] = 1
	_select_raises(ctx, 'segment outside -1 .. n_seg - 1', seg=bad)
	bad[1, 3] = -2
	_select_raises(ctx, 'segment outside -1 .. n_seg - 1', seg=bad)
	_select_raises(ctx, 'h_prob_off must rise', prob_off=(0, 2, 1))
	_select_raises(ctx, 'h_prob_off must start at 0', prob_off=(1, 2, 3))
