# -*- coding: utf-8 -*-
"""
Halo photometry in the batched frames entry (csrc/halo_stack.hip: select / gather / outputs on the device; ``halo.photometry_frames``,
``pipeline.halo_frames``, the switch of ``tessphot_frames``) against the restatement (tests/halo_common.py), against the
per-target plugin path on host cubes cut from the same frames, and against ``tessphot(None, ...)``.
"""
import numpy as np
import pytest
import halo_common as hc
import halo_frames_common as fc

pytestmark = pytest.mark.gpu

NPIX = (1, 63, 64, 484, 1257)
NCAD = (3, 1299, 1300, 19000)
#: flux_err: up to 4 096 non-negative float64 terms summed in another order than numpy's nansum
FLUX_ERR_RTOL = 4096 * 2.0**-53


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _settings_on(monkeypatch, tmp_path):
	ini = tmp_path / 'settings.ini'
	ini.write_text('[halo]\nenabled = true\n')
	monkeypatch.setenv('TESSPHOT_SETTINGS', str(ini))


def _stack(ctx, frames, row0, col0):
	from photometry_amd.pipeline import FrameStack
	return FrameStack(ctx, {k: np.ascontiguousarray(np.moveaxis(v, 2, 0)) for k, v in frames.items()}, row0, col0)


def _cut(frames, name, st, row0, col0):
	return np.ascontiguousarray(frames[name][st[0] - row0:st[1] - row0, st[2] - col0:st[3] - col0])


def _check_problems(fp, cubes, masks, quality, seg, label):
	"""pix, cad, fit equal, P bit-equal, padding zero -- against halo_common.problems, target by target."""
	dev = fp.gather().to_host()
	for j in range(fp.n):
		ref = hc.problems(cubes[j], quality, masks[j], seg)
		assert len(ref) == fp.n_seg
		for k, r in enumerate(ref):
			d = dev[j * fp.n_seg + k]
			np.testing.assert_array_equal(d['pix'], r['pix'], err_msg=f'{label} target {j} segment {k}')
			np.testing.assert_array_equal(d['cad'], r['cad'], err_msg=f'{label} target {j} segment {k}')
			np.testing.assert_array_equal(d['fit'], r['fit'], err_msg=f'{label} target {j} segment {k}')
			if d['P'] is None:      # a target with a segment without pixels is not packed
				assert not fp.usable[j] and any(len(x['pix']) == 0 for x in ref)
				continue
			npix = len(r['pix'])
			assert d['P'].shape == (len(r['cad']), (npix + 3) // 4 * 4)
			assert np.array_equal(d['P'][:, :npix].view('uint32'), r['P'].view('uint32')), f'{label} target {j} segment {k}'
			assert not d['P'][:, npix:].any()


def test_select_and_gather_on_the_region(ctx):
	from photometry_amd import halo
	frames, row0, col0, time, quality, cat, targets = fc.region()
	stack = _stack(ctx, frames, row0, col0)
	T = len(time)
	seg = halo.segments(time, halo.split_times(2, time, np.zeros(T)))
	stamps, valid = halo.frames_stamps(stack.limits, targets)
	assert valid.all()
	for i in range(len(stamps)):
		assert tuple(stamps[i]) == fc.halo_stamp(stack.limits, targets['row'][i], targets['column'][i])
	checked = 0
	keys = (stamps[:, 1] - stamps[:, 0]) * 1000 + stamps[:, 3] - stamps[:, 2]
	from oracle import sumimage as osum
	for key in np.unique(keys):
		idx = np.flatnonzero(keys == key)
		masks = halo.frames_pixel_masks(ctx, stack, stamps[idx], targets['row'][idx], targets['column'][idx], quality)
		cubes = [_cut(frames, 'images', stamps[i], row0, col0) for i in idx]
		for j, i in enumerate(idx):
			ref = hc.pixel_mask(np.isfinite(osum.sumimage(cubes[j], quality)).astype('int32'), tuple(stamps[i]), targets['row'][i], targets['column'][i])
			np.testing.assert_array_equal(masks[j], ref)
		fp = halo.FramesProblems(ctx, stack, stamps[idx], masks, seg, quality)
		_check_problems(fp, cubes, masks, quality, seg, f'region {key}')
		fp.free()
		checked += len(idx)
	assert checked == len(stamps)


#: (ncad, stamp side, mask sizes): the shapes of the solver's tests on 36 x 36 stamps, and the stamp limit: 64 x 64 = 4096 pixels with
#: masks of 2049 pixels and of all of them, two segments of one full and one partial select tile each
SYNTHETIC = [pytest.param(ncad, 36, NPIX, id=str(ncad)) for ncad in NCAD] + [pytest.param(130, 64, (2049, 4096), id='130-64x64')]


@pytest.mark.parametrize('ncad,side,npixs', SYNTHETIC)
def test_select_and_gather_on_synthetic_stamps(ctx, ncad, side, npixs):
	from photometry_amd import halo
	from photometry_amd.pipeline import FrameStack
	rng = np.random.default_rng(ncad)
	H = W = side
	n = len(npixs)
	R, C = H, W * n
	images = rng.uniform(50, 1000, (ncad, R, C)).astype('float32')
	images[rng.random(images.shape) < 2e-5] = np.nan
	images[rng.random(images.shape) < 1e-5] = np.inf
	images[rng.random(images.shape) < 1e-5] = -np.inf
	# pixels below, at and around minflux: every column 5 of a stamp far below, column 7 scattered round -100, column 9 exactly -100
	for j in range(n):
		images[:, 3:9, j * W + 5] = -500.0 + rng.normal(size=(ncad, 6)).astype('float32')
		images[:, :, j * W + 7] = (-100.0 + rng.normal(size=(ncad, R))).astype('float32')
		images[:, 10:14, j * W + 9] = -100.0
		images[::2, 20, j * W + 9] = -100.5
		images[1::2, 20, j * W + 9] = -99.5
	quality = np.where(rng.random(ncad) < 0.05, 32, 0).astype('int32')
	seg = np.zeros(ncad, dtype='int64') if ncad <= 3 else (np.arange(ncad) >= ncad // 2 + 1).astype('int64')
	if ncad > 3:
		seg[rng.choice(ncad, size=3, replace=False)] = -1
		seg[-1] = 1
	stamps = np.array([[100, 100 + H, 200 + j * W, 200 + (j + 1) * W] for j in range(n)], dtype='int64')
	masks = np.zeros((n, H, W), dtype=bool)
	for j, npix in enumerate(npixs):
		masks[j].ravel()[rng.choice(H * W, size=npix, replace=False)] = True
		if npix >= 63:
			masks[j][3:9, 5] = masks[j][:8, 7] = masks[j][10:14, 9] = masks[j][20, 9] = True
	# (only the image stack is read by select / gather: the other two are not made)
	stack = FrameStack.__new__(FrameStack)
	stack.ctx, stack.row0, stack.col0 = ctx, 100, 200
	stack.dev = {'images': ctx.array(images)}
	stack.n_cad, stack.n_rows, stack.n_cols = images.shape
	stack.limits = (100, 100 + R, 200, 200 + C)
	fp = halo.FramesProblems(ctx, stack, stamps, masks, seg, quality)
	cubes = [np.ascontiguousarray(np.moveaxis(images[:, :, j * W:(j + 1) * W], 0, 2)) for j in range(n)]
	_check_problems(fp, cubes, masks, quality, seg, f'synthetic T={ncad}')
	print(f"synthetic T={ncad}: npix {fp.npix.tolist()} of masks {[int(m.sum()) for m in masks]}, ncad {fp.ncad.tolist()}")
	assert np.any(fp.npix < np.array([m.sum() for m in masks])[:, None]) or ncad <= 3
	if side == 64:
		assert fp.npix.max() > 3072 and fp.ncad.min() > 32, (fp.npix.tolist(), fp.ncad.tolist())
	fp.free()
	stack.dev['images'].free()


def test_a_segment_without_cadences(ctx):
	"""Sector 1 has three split times; a region with no frame between two of them has an empty segment: every mask pixel is kept,
	no cadence, a degenerate problem -- an error of the target, not of the call, as on the per-target path."""
	from photometry_amd import halo, pipeline, STATUS
	from photometry_amd.plugins import load_settings, mag2flux
	frames, row0, col0, time, quality, cat, targets = fc.region()
	T = len(time)
	time = np.where(np.arange(T) < T // 2, 1346.9 + np.arange(T) * 0.02, 1349.4 + np.arange(T) * 0.02)   # nothing in (1347.366, 1349.315)
	stack = _stack(ctx, frames, row0, col0)
	seg = halo.segments(time, halo.split_times(1, time, np.zeros(T)))
	assert seg.max() == 2 and not np.any(seg == 1)
	i = int(np.flatnonzero(targets['starid'] == fc.BRIGHT_KEPT)[0])
	stamps, _ = halo.frames_stamps(stack.limits, targets)
	masks = halo.frames_pixel_masks(ctx, stack, stamps[i:i + 1], targets['row'][i:i + 1], targets['column'][i:i + 1], quality)
	fp = halo.FramesProblems(ctx, stack, stamps[i:i + 1], masks, seg, quality)
	_check_problems(fp, [_cut(frames, 'images', stamps[i], row0, col0)], masks, quality, seg, 'empty segment')
	assert fp.npix[0, 1] == masks[0].sum() and fp.ncad[0, 1] == 0
	fp.free()
	settings = load_settings()
	settings.set('halo', 'enabled', 'true')
	one = {k: v[i:i + 1] for k, v in targets.items()}
	res = pipeline.halo_frames(ctx, stack, one, cat, time, quality, sector=1, settings=settings)
	assert res.status[0] == STATUS.ERROR.value and res.errors[0] == ['ERROR: Halo optimization failed']
	ref = halo.photometry(ctx, _cut(frames, 'images', stamps[i], row0, col0), _cut(frames, 'images_err', stamps[i], row0, col0), quality, time,
		np.zeros(T), np.arange(T), masks[0], 1, mag2flux(targets['tmag'][i]))
	assert np.array_equal(res.tv_status[0], ref['status']) and ref['status'][1] == halo.DEGENERATE
	assert _same_bits(res.corr_flux[0], ref['corr_flux'])
	assert np.all(np.abs(res.flux_err[0] - ref['flux_err']) <= FLUX_ERR_RTOL * np.abs(ref['flux_err']))
	for a, b in zip(halo.photometry_frames(ctx, stack, one, time, quality, sector=1)['weightmap'][0], ref['weightmap']['weightmap']):
		assert np.array_equal(a, b, equal_nan=True)


def _reference(ctx, frames, row0, col0, time, quality, tmag, stamp, mask, cadenceno=None):
	"""The parent path: the cube cut on the host, ``halo.photometry``."""
	from photometry_amd import halo
	from photometry_amd.plugins import mag2flux
	T = len(time)
	return halo.photometry(ctx, _cut(frames, 'images', stamp, row0, col0), _cut(frames, 'images_err', stamp, row0, col0), quality, time,
		np.zeros(T), np.arange(T) if cadenceno is None else cadenceno, mask, 2, mag2flux(tmag))


def _same_bits(a, b):
	a, b = np.asarray(a), np.asarray(b)
	return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view('uint64') if a.dtype == np.float64 else a,
		b.view('uint64') if b.dtype == np.float64 else b)


def _assert_equals_reference(res, i, ref, label):
	assert _same_bits(res.corr_flux[i], ref['corr_flux']), label
	assert _same_bits(res.flux[i], ref['flux']), label
	assert _same_bits(res.f[i], ref['f']) and np.array_equal(res.iterations[i], ref['iterations']) and np.array_equal(res.tv_status[i], ref['status']), label
	assert len(res.w[i]) == len(ref['w'])
	for a, b in zip(res.w[i], ref['w']):
		assert _same_bits(a, b), label
	wm = res.weightmap[i]
	assert wm['initial_cadence'] == ref['weightmap']['initial_cadence'] and wm['final_cadence'] == ref['weightmap']['final_cadence']
	assert wm['sat_pixels'] == ref['weightmap']['sat_pixels']
	for a, b in zip(wm['weightmap'], ref['weightmap']['weightmap']):
		assert _same_bits(a, b), label
	err = np.abs(res.flux_err[i] - ref['flux_err'])
	worst = float(np.max(err / np.where(ref['flux_err'] > 0, ref['flux_err'], 1.0)))
	print(f"{label}: worst relative flux_err difference {worst:.3e} (bound {FLUX_ERR_RTOL:.3e})")
	assert np.all(err <= FLUX_ERR_RTOL * np.abs(ref['flux_err'])), (label, worst)
	return worst


@pytest.fixture(scope='module')
def region_run(ctx):
	from photometry_amd import pipeline
	from photometry_amd.plugins import load_settings
	frames, row0, col0, time, quality, cat, targets = fc.region()
	stack = _stack(ctx, frames, row0, col0)
	settings = load_settings()
	settings.set('halo', 'enabled', 'true')
	res = pipeline.halo_frames(ctx, stack, targets, cat, time, quality, sector=2, settings=settings)
	return {'frames': frames, 'row0': row0, 'col0': col0, 'time': time, 'quality': quality, 'cat': cat, 'targets': targets, 'stack': stack,
		'settings': settings, 'res': res}


def test_halo_frames_equals_the_per_target_path(ctx, region_run):
	from photometry_amd import STATUS
	g = region_run
	res, targets = g['res'], g['targets']
	assert res.split_times == (1368.0,) and res.f.shape[1] == 2
	worst = 0.0
	for i in range(len(res)):
		assert res.status[i] == STATUS.OK.value, (i, res.errors.get(i))
		ref = _reference(ctx, g['frames'], g['row0'], g['col0'], g['time'], g['quality'], targets['tmag'][i], res.stamp[i], res.pixel_mask[i])
		worst = max(worst, _assert_equals_reference(res, i, ref, f"target {targets['starid'][i]}"))
		np.testing.assert_array_equal(res.pos_centroid[i, :, 0], targets['column'][i])
		np.testing.assert_array_equal(res.pos_centroid[i, :, 1], targets['row'][i])
		assert res.diagnostics[i] is not None and np.isfinite(res.diagnostics[i]['mean_flux'])
	print(f"halo_frames against halo.photometry: worst relative flux_err difference over the region {worst:.3e}")
	first = int(np.flatnonzero(targets['starid'] == fc.BRIGHT_SWITCHING[0])[0])
	assert res.skip_targets[first] == [fc.NEIGHBOUR]
	assert res.headers['HALO_OBJ'][0] == 'tv' and res.headers['HALO_MXI'][0] == 101


def test_off_by_default(ctx, region_run, monkeypatch):
	from photometry_amd import pipeline
	g = region_run
	monkeypatch.delenv('TESSPHOT_SETTINGS', raising=False)
	with pytest.raises(NotImplementedError, match=r'\[halo\] enabled = true'):
		pipeline.halo_frames(ctx, g['stack'], g['targets'], g['cat'], g['time'], g['quality'], sector=2)


def _assert_same_result(a, i, b, j):
	assert a.status[i] == b.status[j] and tuple(a.stamp[i]) == tuple(b.stamp[j])
	for name in ('flux', 'flux_err', 'corr_flux', 'f'):
		assert _same_bits(getattr(a, name)[i], getattr(b, name)[j]), name
	assert np.array_equal(a.iterations[i], b.iterations[j]) and np.array_equal(a.tv_status[i], b.tv_status[j])
	for x, y in zip(a.w[i], b.w[j]):
		assert _same_bits(x, y)
	for x, y in zip(a.weightmap[i]['weightmap'], b.weightmap[j]['weightmap']):
		assert _same_bits(x, y)


def test_reproducible_batch_independent_and_chunked(ctx, region_run):
	from photometry_amd import pipeline
	g = region_run
	res, targets = g['res'], g['targets']
	n = len(res)
	call = lambda t, **kw: pipeline.halo_frames(ctx, g['stack'], t, g['cat'], g['time'], g['quality'], sector=2, settings=g['settings'], **kw)
	again = call(targets)
	for i in range(n):
		_assert_same_result(again, i, res, i)
	for i in (0, 3, n - 1):
		alone = call({k: v[i:i + 1] for k, v in targets.items()})
		_assert_same_result(alone, 0, res, i)
	# a budget that holds one, then three, 23 x 23 stamps (the largest of the region): chunks of targets
	bound = 4 * ((23 * 23 + 3) // 4 * 4) * len(g['time'])
	for k in (1, 3):
		chunked = call(targets, budget_bytes=k * bound)
		for i in range(n):
			_assert_same_result(chunked, i, res, i)


def test_degenerate_and_unusable_targets_do_not_disturb_the_batch(ctx, region_run):
	from photometry_amd import pipeline, STATUS
	g = region_run
	frames = {k: v.copy() for k, v in g['frames'].items()}
	targets, row0, col0 = g['targets'], g['row0'], g['col0']
	at = lambda sid: int(np.flatnonzero(targets['starid'] == sid)[0])
	deg, unusable = at(fc.BRIGHT_SWITCHING[1]), at(fc.BRIGHT_SWITCHING[2])
	st = g['res'].stamp[deg]
	frames['images'][st[0] - row0 + 3, st[2] - col0 + 4, :10] = np.nan       # 10 of the 12 cadences of segment 0 lose a kept pixel
	st = g['res'].stamp[unusable]
	frames['images'][st[0] - row0:st[1] - row0, st[2] - col0:st[3] - col0, :] = -500.0    # every mask pixel below minflux
	stack = _stack(ctx, frames, row0, col0)
	# the four bright targets as one batch (the stamps of the other two bright ones hold no changed pixel)
	bright = np.array([at(sid) for sid in fc.BRIGHT_SWITCHING + (fc.BRIGHT_KEPT,)])
	res = pipeline.halo_frames(ctx, stack, {k: v[bright] for k, v in targets.items()}, g['cat'], g['time'], g['quality'], sector=2, settings=g['settings'])
	assert res.status[1] == STATUS.ERROR.value and res.errors[1] == ['ERROR: Halo optimization failed']
	assert res.status[2] == STATUS.ERROR.value and res.errors[2][0].endswith('Halo photometry: no usable pixels in the pixel mask')
	for j in (0, 3):
		assert res.status[j] == STATUS.OK.value
		_assert_same_result(res, j, g['res'], bright[j])


def test_known_answer_bright_star(ctx, region_run):
	from photometry_amd import pipeline, STATUS
	from photometry_amd.plugins import mag2flux
	sc = hc.bright_star_scene()
	stack = _stack(ctx, sc['frames'], sc['row0'], sc['col0'])
	tg = {k: np.asarray(v)[:1] for k, v in sc['targets'].items()}
	res = pipeline.halo_frames(ctx, stack, tg, sc['catalog'], sc['time'], sc['quality'], sector=2, timecorr=sc['timecorr'], cadenceno=sc['cadenceno'],
		jitter=sc['jitter'], settings=region_run['settings'])
	assert res.status[0] == STATUS.OK.value, res.errors
	assert res.split_times == (1368.0,) and len(res.w[0]) == 2
	corr = res.flux[0] / mag2flux(5.0)
	seg = res.segments
	amp, rms = hc.sinusoid_fit(sc['time'], corr, seg, sc['period'])
	st = res.stamp[0]
	cube = sc['frames']['images'][st[0] - sc['row0']:st[1] - sc['row0'], st[2] - sc['col0']:st[3] - sc['col0']]
	s = cube[res.pixel_mask[0]].astype('float64').sum(axis=0)
	plain = np.full(len(s), np.nan)
	good = (sc['quality'] & hc.DEFAULT_BITMASK) == 0
	for k in range(seg.max() + 1):
		plain[seg == k] = s[seg == k] / np.median(s[(seg == k) & good])
	amp0, rms0 = hc.sinusoid_fit(sc['time'], plain, seg, sc['period'])
	print(f"known answer through halo_frames: amplitude {amp:.4e} (injected 1e-3), residual rms {rms:.3e} vs plain sum {rms0:.3e}")
	assert abs(amp - 1e-3) <= 0.1e-3
	assert rms <= 0.5 * rms0
	np.testing.assert_allclose(res.pos_centroid[0, :, 0], sc['targets']['column'][0] + sc['jitter'][:, 0])
	assert res.weightmap[0]['initial_cadence'][0] == 1000


def test_tessphot_frames_switches_like_tessphot(ctx, region_run, monkeypatch, tmp_path):
	from photometry_amd import tessphot, tessphot_frames, tessphot_frames_pipelined, pipeline, STATUS
	from photometry_amd.plugins import HaloPhotometry
	from photometry_amd.source import MemoryStampSource
	g = region_run
	frames, row0, col0, time, quality, cat, targets, stack = (g[k] for k in ('frames', 'row0', 'col0', 'time', 'quality', 'cat', 'targets', 'stack'))
	T, n = len(time), len(targets['starid'])
	# Halo off: the parent's result
	monkeypatch.delenv('TESSPHOT_SETTINGS', raising=False)
	off = tessphot_frames(ctx, stack, targets, cat, time, quality, sector=2)
	plain = pipeline.aperture_frames(ctx, stack, targets, cat, time, quality)
	assert not off.halo_rows and np.array_equal(off.frames.status, plain.status) and np.array_equal(off.stamp, plain.stamp)
	off_items = [off[i] for i in range(n)]
	for i in range(n):
		a, b = off_items[i], plain[i]
		assert a.method == 'aperture' and a.halo_weightmap is None and a._details.get('errors', []) == b['errors']
		assert a.status.value == off.status[i] and tuple(a._details['stamp']) == tuple(b['stamp']) and a._details['stamp_resizes'] == b['stamp_resizes']
		if 'mask' in b:
			for key in ('flux', 'flux_err', 'flux_background', 'pos_centroid'):
				assert _same_bits(a.lightcurve[key], b[key]), (i, key)
			np.testing.assert_array_equal(a.final_phot_mask, b['mask'])
			assert a._details['mask_size'] == int(b['mask'].sum()) and a._details.get('skip_targets', []) == b['skip_targets']
			assert a._details.get('contamination', np.nan) == b['contamination'] or np.isnan(b['contamination'])
			if a.status in (STATUS.OK, STATUS.WARNING):
				for key in ('mean_flux', 'variance', 'rms_hour', 'ptp', 'variability', 'edge_flux'):
					assert a._details[key] == float(b['diagnostics'][key]) or np.isnan(a._details[key]), (i, key)
		else:
			assert a.lightcurve is None and a.final_phot_mask is None
			if 'edge_flux' in b:
				assert a._details['edge_flux'] == b['edge_flux']
	# Halo on
	_settings_on(monkeypatch, tmp_path)
	on = tessphot_frames(ctx, stack, targets, cat, time, quality, sector=2)
	switched = sorted(int(targets['starid'][i]) for i in on.halo_rows)
	for i in on.halo_rows:
		assert tuple(on.stamp[i]) == tuple(on[i]._details['stamp']) and on.status[i] == on[i].status.value
	assert tuple(switched) == fc.BRIGHT_SWITCHING
	for i in range(n):
		sid = int(targets['starid'][i])
		src = MemoryStampSource(frames, row0, col0, time, np.zeros(T), np.arange(T), quality, cat, sector=2, targets=targets)
		pho = tessphot(None, sid, src, str(tmp_path / f'out{sid}'), ctx=ctx)
		b = on[i]
		assert b.method == pho.method and b.status == pho.status == STATUS(int(on.status[i])), (sid, b.method, pho.method, b.status, pho.status)
		assert tuple(b._details['stamp']) == tuple(pho._details['stamp']), sid
		if i in on.halo_rows:
			assert isinstance(pho, HaloPhotometry) and b.method == 'halo'
			assert 'Automatically switched to Halo photometry' in b._details['errors'] and 'Automatically switched to Halo photometry' in pho._details['errors']
			assert b._details['edge_flux'] == pho._details['edge_flux'] and b._details['edge_flux'] is not None
			assert _same_bits(b.lightcurve['flux'], np.asarray(pho.lightcurve['flux'], dtype='float64')), sid
			assert _same_bits(b.lightcurve['pos_centroid'], np.asarray(pho.lightcurve['pos_centroid'], dtype='float64')), sid
			assert _same_bits(b.lightcurve['flux_background'], np.asarray(pho.lightcurve['flux_background'], dtype='float64')), sid
			ref = np.asarray(pho.lightcurve['flux_err'])
			assert np.all(np.abs(b.lightcurve['flux_err'] - ref) <= FLUX_ERR_RTOL * np.abs(ref)), sid
			np.testing.assert_array_equal(b.final_phot_mask, pho.final_phot_mask)
			assert b.halo_weightmap['initial_cadence'] == pho.halo_weightmap['initial_cadence']
			assert b.halo_weightmap['final_cadence'] == pho.halo_weightmap['final_cadence']
			for x, y in zip(b.halo_weightmap['weightmap'], pho.halo_weightmap['weightmap']):
				assert _same_bits(x, y), sid
			assert b._details.get('skip_targets') == pho._details.get('skip_targets')
			for key in ('mean_flux', 'variance', 'ptp', 'mask_size'):
				assert b._details[key] == pho._details[key], (sid, key)
		else:
			a = off_items[i]
			assert b.method == 'aperture' and b.status == a.status and b._details.get('errors', []) == a._details.get('errors', [])
			if a.lightcurve is not None:
				for key in ('flux', 'flux_err', 'flux_background', 'pos_centroid'):
					assert _same_bits(b.lightcurve[key], a.lightcurve[key]), (sid, key)
				np.testing.assert_array_equal(b.final_phot_mask, a.final_phot_mask)
	# the pipelined entry yields the same
	halves = [{k: v[:4] for k, v in targets.items()}, {k: v[4:] for k, v in targets.items()}]
	got = list(tessphot_frames_pipelined(ctx, stack, halves, cat, time, quality, sector=2))
	assert len(got) == 2
	for h, part in enumerate(got):
		for j in range(len(part)):
			i = 4 * h + j
			a, b = part[j], on[i]
			assert a.method == b.method and a.status == b.status and a._details.get('errors', []) == b._details.get('errors', [])
			if b.lightcurve is not None:
				for key in ('flux', 'flux_err', 'pos_centroid'):
					assert _same_bits(a.lightcurve[key], b.lightcurve[key]), (i, key)
			if b.method == 'halo':
				for x, y in zip(a.halo_weightmap['weightmap'], b.halo_weightmap['weightmap']):
					assert _same_bits(x, y)


@pytest.mark.parametrize('T', (64, 256, 65, 257))
def test_norm_median_on_heavy_ties(ctx, monkeypatch, T):
	"""The norm kernel's selection (the block selection shared with the solver's stat kernel, 256 threads) on a light curve of a few
	values with many copies each: frames periodic in time (period 4 for an even count of fitted cadences -- the two middle ranks fall
	on different values -- and 5 for an odd one), one 6 x 6 stamp with the full mask inside a 12 x 12 stack, one segment, cadences
	8 .. 11 not fitted.  ``halo.photometry`` takes numpy's median of the same ``l``: corr_flux and the weight map must equal it bit
	for bit."""
	from photometry_amd import halo
	from photometry_amd.plugins import mag2flux
	rng = np.random.default_rng(T)
	period = 4 if T % 2 == 0 else 5
	R = C = 12
	base = rng.uniform(50, 1000, (R, C, period)).astype('float32')
	frames = {'images': np.ascontiguousarray(base[:, :, np.arange(T) % period]), 'images_err': rng.uniform(1, 2, (R, C, T)).astype('float32'),
		'backgrounds': np.zeros((R, C, T), dtype='float32')}
	row0, col0 = 100, 200
	stamp = np.array([[row0 + 3, row0 + 9, col0 + 2, col0 + 8]], dtype='int64')
	mask = np.ones((6, 6), dtype=bool)
	time = 1500.0 + np.arange(T) * 1800.0 / 86400.0
	quality = np.zeros(T, dtype='int32')
	quality[8:12] = 32
	targets = {'starid': np.array([1], dtype='int64'), 'tmag': np.array([5.0]), 'row': np.array([row0 + 6.0]), 'column': np.array([col0 + 5.0])}
	stack = _stack(ctx, frames, row0, col0)
	monkeypatch.setattr(halo, 'frames_stamps', lambda limits, tg: (stamp, np.ones(1, dtype=bool)))
	monkeypatch.setattr(halo, 'frames_pixel_masks', lambda *a, **k: mask[None])
	got = halo.photometry_frames(ctx, stack, targets, time, quality)
	assert got['segments'].max() == 0 and got['usable'][0] and got['npix'][0, 0] == 36 and got['ncad'][0, 0] == T
	assert got['status'][0, 0] != halo.DEGENERATE
	cube, cube_err = _cut(frames, 'images', stamp[0], row0, col0), _cut(frames, 'images_err', stamp[0], row0, col0)
	# the device's fitted l: as many distinct values as the period, with T / period copies each
	prob = halo.build_problems(cube, quality, mask, got['segments'])
	dev = halo.tvmin(ctx, prob)
	fitted = dev['l'][0][prob[0].fit]
	assert len(fitted) == T - 4 and len(np.unique(fitted)) <= 6
	assert _same_bits(got['w'][0][0], dev['w'][0]) and got['iterations'][0, 0] == dev['iterations'][0]
	ref = halo.photometry(ctx, cube, cube_err, quality, time, np.zeros(T), np.arange(T), mask, -1, mag2flux(5.0))
	assert ref['status'][0] == got['status'][0, 0]
	assert _same_bits(got['corr_flux'][0], ref['corr_flux'])
	assert _same_bits(got['weightmap'][0][0], ref['weightmap']['weightmap'][0])
