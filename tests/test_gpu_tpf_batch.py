# -*- coding: utf-8 -*-
"""
``tessphot_tpfs``: a batch of target pixel files against the per-file call it stands for, ``tessphot('aperture', starid,
TpfStampSource(load_tpfs(...)[0], catalog, targets), output, datasource='tpf')``, on the same device.

Six files written from ``simulate`` scenes the way tests/test_gpu_tpf_load.py writes its one: four of 11 x 11 x 70 that share a shape
and nothing else -- a regular time axis; one with a gap and cadences flagged by the default bitmask (its sum image moves);
``DATA_REL = 20`` (the time offset) with another shift and flags outside the bitmask; a ``FLUX`` that is all NaN -- one 11 x 11 with
two rows of non-finite ``TIME`` (68 cadences) and one of 9 x 13.  Every result is held to the plugin's: status, every light-curve
column bit for bit, mask and sum image, the details key by key (floats by their bits; a traceback by its last line, which is what
the batched entries keep of an exception), the light-curve files HDU by HDU as tests/test_gpu_lightcurve_files.py compares them.
The batch may say more than the plugin in two places, as ``BatchResults`` does: ``stamp_resizes`` (always 0 here), and ``mask_size``
/ ``contamination`` of a target that ends in ERROR after its mask was made.
"""
import os
import numpy as np
import pytest
import ffi_common as fc
import tpf_common as tc
from photometry_amd import tpf, tessphot, tessphot_tpfs, STATUS
from test_gpu_lightcurve_files import _hold_files

pytestmark = pytest.mark.gpu

H = W = 11
T = 70
VERSION = 6
CADENCE = 120.0 / 86400.0


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _bits_equal(a, b):
	a, b = np.asarray(a), np.asarray(b)
	return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view('uint8'), np.ascontiguousarray(b).view('uint8'))


def _write(root, s, i, rng, starid_offset=0, time=None, quality=None, bad_times=(), primary=None, all_nan=False):
	"""Target ``i`` of the scene ``s`` as a target pixel file; returns ``(path, starid)``."""
	h, w, n = s.height, s.width, s.n_cad
	st = tuple(int(v) for v in s.stamps[i])
	cubes = {'FLUX': np.moveaxis(s.images[i], 2, 0).copy(), 'FLUX_ERR': np.moveaxis(s.images_err[i], 2, 0).copy(), 'FLUX_BKG': np.moveaxis(s.backgrounds[i], 2, 0).copy()}
	ap = np.ones((h, w), dtype='int32')
	ap[3:8, 3:8] |= 2
	ap[4:7, 4:7] |= 8
	ap[:, :6] |= 32
	ap[:, 6:] |= 64
	ap[0, 0] &= ~1                                                            # a pixel never collected: NaN flux, bit 1 clear
	cubes['FLUX'][:, 0, 0] = np.nan
	cubes['FLUX_ERR'][:, 0, 0] = np.nan
	if all_nan:
		cubes['FLUX'][:] = np.nan
	time = np.array(s.time if time is None else time, dtype='float64')
	time[list(bad_times)] = np.nan                                            # (make_tpf's own bad_times are overwritten by the scalars)
	scalars = {'TIME': time, 'TIMECORR': (3e-3 + 1e-5 * rng.normal(size=n)).astype('float32'),
		'QUALITY': s.quality if quality is None else quality, 'POS_CORR1': s.jitter[:, 0].astype('float32'), 'POS_CORR2': s.jitter[:, 1].astype('float32')}
	starid = int(s.target_starid[i]) + starid_offset
	blob, rec, ap_file, info = tc.make_tpf(rng, h, w, n, crval1p=st[2] + 1, crval2p=st[0] + 1, aperture=ap, images=cubes, scalars=scalars, bad_times=bad_times,
		primary=dict(TICID=starid, **(primary or {})))
	return fc.write(root / ('tess2019199201929-s0014-%016d-0150-s_tp.fits' % starid), blob), starid


@pytest.fixture(scope='module')
def six(tmp_path_factory):
	from photometry_amd import simulate
	root = tmp_path_factory.mktemp('tpfbatch')
	rng = np.random.default_rng(61)
	a = simulate.make_scene(5, T, H, W, seed=12, cadence_s=120.0)
	simulate.fill_cubes(a, nan_fraction=0.0)
	b = simulate.make_scene(1, T, 9, 13, seed=13, cadence_s=120.0)
	simulate.fill_cubes(b, nan_fraction=0.0)
	gap = a.time.copy()
	gap[T // 2:] += 0.5 - CADENCE
	flagged = np.zeros(T, dtype='int32')
	flagged[[3, 4, 5, 20, 41, 42, 60]] = [1, 2, 4, 8, 32, 128, 4096]                # all in the default bitmask
	outside = np.zeros(T, dtype='int32')
	outside[[7, 30]] = 16                                                       # bit 16 is not
	made = [_write(root, a, 0, rng), _write(root, a, 1, rng, time=gap, quality=flagged),
		_write(root, a, 2, rng, time=a.time + 0.3, quality=outside, primary=dict(DATA_REL=20, PROCVER='spoc-4.0.5-20190101')),
		_write(root, a, 3, rng, bad_times=(33, 34)), _write(root, b, 0, rng, starid_offset=1000), _write(root, a, 4, rng, all_nan=True)]
	# one catalogue for all files: every scene's stars, the second scene's star numbers moved out of the first one's way
	cat = {k: np.concatenate((a.catalog[k], b.catalog[k])) for k in ('starid', 'tmag', 'row', 'column')}
	cat['starid'] = np.concatenate((a.catalog['starid'], b.catalog['starid'] + 1000))
	targets = {'starid': np.concatenate((a.target_starid, b.target_starid + 1000)), 'tmag': np.concatenate((a.target_tmag, b.target_tmag)),
		'row': np.concatenate((a.target_pos_row, b.target_pos_row)), 'column': np.concatenate((a.target_pos_column, b.target_pos_column))}
	flagged_images = a.images[1].copy()
	flagged_images[0, 0, :] = np.nan                                            # (the pixel _write takes out of every file)
	return {'files': [m[0] for m in made], 'starid': [m[1] for m in made], 'catalog': cat, 'targets': targets, 'nan_file': 5, 'flagged_file': 1, 'plain_file': 0,
		'flagged_images': flagged_images}


@pytest.fixture(scope='module')
def plugin(ctx, six, tmp_path_factory):
	"""The per-file call for every file, once: ``(pho, sum image)`` and the folder its files went to."""
	out = tmp_path_factory.mktemp('plugin')
	res = []
	for path, starid in zip(six['files'], six['starid']):
		(ld,) = tpf.load_tpfs(ctx, [path])
		pho = tessphot('aperture', starid, tpf.TpfStampSource(ld, six['catalog'], targets=six['targets']), str(out), datasource='tpf', ctx=ctx, version=VERSION)
		res.append((pho, None if pho._sumimage is None else np.array(pho._sumimage)))
		ld.free()
	return res, str(out)


@pytest.fixture(scope='module')
def batch(ctx, six, tmp_path_factory):
	"""One chunk with files written, under the kernel profile."""
	out = tmp_path_factory.mktemp('batch')
	ctx.profile(True)
	ctx.profile_reset()
	chunks = list(tessphot_tpfs(ctx, six['files'], six['catalog'], targets=six['targets'], output_folder=str(out), version=VERSION))
	ctx.sync()
	report = ctx.profile_report()
	ctx.profile(False)
	assert len(chunks) == 1
	return chunks[0], str(out), report


def _last_lines(errors):
	return [str(e).strip().splitlines()[-1] for e in errors]


def _same_detail(key, a, b):
	if key == 'errors':
		return _last_lines(a) == _last_lines(b)
	if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
		return _bits_equal(np.asarray(a, dtype='float64'), np.asarray(b, dtype='float64'))
	if isinstance(a, float) or isinstance(b, float):
		return _bits_equal(np.float64(a), np.float64(b))
	return type(a) == type(b) and a == b


def _hold_result(r, pho, sumimage, batch_sum, label):
	assert r.status == pho.status, (label, r.status, pho.status, r._details, pho._details)
	assert r.method == 'aperture' and r.starid == pho.starid
	ok = pho.status in (STATUS.OK, STATUS.WARNING)
	if ok:
		assert list(r.lightcurve.keys()) == list(pho.lightcurve.keys()), label
	if r.lightcurve is not None:
		for key in r.lightcurve.keys():
			assert _bits_equal(r.lightcurve[key], pho.lightcurve[key]), (label, key)
		assert _bits_equal(r.final_phot_mask, pho.final_phot_mask), label
		assert _bits_equal(batch_sum, sumimage), label
	else:
		assert not ok and pho.final_phot_mask is None, label
	mine, theirs = dict(r._details), dict(pho._details)
	for key, value in theirs.items():
		assert key in mine and _same_detail(key, mine[key], value), (label, key, mine.get(key), value)
	extra = set(mine) - set(theirs)
	assert extra <= ({'stamp_resizes'} if ok else {'stamp_resizes', 'mask_size', 'contamination', 'skip_targets'}), (label, extra)
	assert mine['stamp_resizes'] == 0


def test_every_result_is_the_plugins(six, plugin, batch):
	res, out, report = batch
	phos, _ = plugin
	n = len(six['files'])
	assert len(res) == n and res.paths == six['files'] and list(res.starid) == six['starid']
	good = 0
	for i in range(n):
		pho, sumimage = phos[i]
		_hold_result(res[i], pho, sumimage, res.sumimage(i), f'file {i}')
		assert res.status[i] == pho.status.value
		good += pho.status in (STATUS.OK, STATUS.WARNING)
	assert good >= 4, [p.status for p, _ in phos]
	k = six['nan_file']
	assert res.status[k] == STATUS.ERROR.value and phos[k][0].status == STATUS.ERROR and res[k].lightcurve is None
	assert _last_lines(res[k]._details['errors']) == ['RuntimeError: K2P2NoFlux: No measured flux in sum-image']
	# the file's own columns are in the light curve, the time offset of the early data release included
	lc = res[2].lightcurve
	assert _bits_equal(lc['time'], res.loaded[2].time) and res.loaded[2].time_offset_corrected and res.loaded[2].data_rel == 20
	assert lc['timecorr'].dtype == np.float64 and _bits_equal(lc['pos_corr'], res.loaded[2].pos_corr) and lc['pos_corr'].shape == (T, 2)
	assert len(res[3].lightcurve['time']) == T - 2
	# flagged cadences moved the sum image of their file: the 2-D quality reached the kernel
	assert not _bits_equal(res.sumimage(six['flagged_file']), res.sumimage(six['plain_file']))
	# columns
	from photometry_amd.engine import DIAGNOSTICS_COLUMNS
	for name in ('mask_size', 'contamination') + tuple(DIAGNOSTICS_COLUMNS):
		col = res.column(name)
		assert col.shape == (n,) and np.isnan(col[k])
	assert res.column('mask_size')[0] == res[0]._details['mask_size'] and res.column('rms_hour')[0] == res[0]._details['rms_hour']


def test_the_flagged_files_sum_image_is_its_own(six, batch):
	"""The guard that a group's per-target quality matters: the flagged file's pixels give another sum image under the quality of the
	file next to it in the cube, and the batch's is the one of its own flags (``oracle.sumimage``, to the 1e-12 of the suite's sum images)."""
	from oracle import sumimage as osum
	res, _, _ = batch
	k = six['flagged_file']
	images = six['flagged_images']
	own = osum.sumimage(images, res.loaded[k].quality)
	other = osum.sumimage(images, res.loaded[six['plain_file']].quality)
	assert np.nanmax(np.abs(own - other)) > 1e-3 * np.nanmax(np.abs(own))
	np.testing.assert_allclose(res.sumimage(k), own, rtol=1e-12, equal_nan=True)


def test_files_written(six, plugin, batch):
	res, out, _ = batch
	phos, plugin_out = plugin
	assert sorted(os.listdir(out)) == sorted(os.listdir(plugin_out))
	wrote = [i for i in range(len(res)) if res.status[i] in (STATUS.OK.value, STATUS.WARNING.value)]
	assert len(os.listdir(out)) == len(wrote) >= 4
	for i in range(len(res)):
		if i in wrote:
			name = os.path.basename(res.filepaths[i])
			assert os.path.dirname(res.filepaths[i]) == out
			assert res[i]._details['filepath_lightcurve'] == phos[i][0]._details['filepath_lightcurve'] == name
			problems = _hold_files(os.path.join(out, name), os.path.join(plugin_out, name), res.sumimage(i), f'file {i}')
			assert not problems, (i, problems)
		else:
			assert res.filepaths[i] is None and 'filepath_lightcurve' not in res[i]._details and 'filepath_lightcurve' not in phos[i][0]._details
	assert any('-dr20-' in os.path.basename(p) for p in res.filepaths if p)


def _launches(report, word):
	return sum(n for name, (n, _ms) in report.items() if word in name)


def test_one_launch_per_group_and_chunks_change_nothing(ctx, six, batch):
	res, _, report = batch
	# the groups of the one chunk: (11, 11, 70) x 4, (11, 11, 68), (9, 13, 70)
	assert _launches(report, 'fused') == 3 and _launches(report, 'diagnostics') == 3, report
	ctx.profile(True)
	ctx.profile_reset()
	chunks = list(tessphot_tpfs(ctx, six['files'], six['catalog'], targets=six['targets'], chunk_files=3))
	ctx.sync()
	report3 = ctx.profile_report()
	ctx.profile(False)
	assert [len(c) for c in chunks] == [3, 3]
	# files 0..2 are one group, files 3..5 three
	assert _launches(report3, 'fused') == 4 and _launches(report3, 'diagnostics') == 4, report3
	flat = [(c, j) for c in chunks for j in range(len(c))]
	for i, (c, j) in enumerate(flat):
		a, b = c[j], res[i]
		assert c.filepaths[j] is None and c.paths[j] == six['files'][i]
		assert a.status == b.status and a.starid == b.starid
		assert (a.lightcurve is None) == (b.lightcurve is None)
		if a.lightcurve is not None:
			for key in b.lightcurve:
				assert _bits_equal(a.lightcurve[key], b.lightcurve[key]), (i, key)
			assert _bits_equal(a.final_phot_mask, b.final_phot_mask) and _bits_equal(c.sumimage(j), res.sumimage(i))
		for key in set(b._details) - {'filepath_lightcurve'}:
			assert _same_detail(key, a._details[key], b._details[key]), (i, key)


def test_a_catalogue_in_ra_dec_goes_through_every_files_own_wcs(ctx, six, tmp_path):
	"""``ra`` / ``dec`` for catalogue and targets: the 11 x 11 files and the 9 x 13 file project them through different WCSs (each relative
	to its own stamp), in one ``tp_wcs_world2pix`` call for the chunk, and the results are the per-file call's."""
	from photometry_amd.wcs import as_wcs
	files = [six['files'][k] for k in (0, 4, 1)]
	starid = [six['starid'][k] for k in (0, 4, 1)]
	(ld,) = tpf.load_tpfs(ctx, files[:1])
	w = as_wcs(ld.wcs_cards, ctx=ctx)
	pix = np.array([[5.2, 4.9], [2.5, 7.5], [8.0, 2.0], [5.1, 5.3], [4.8, 5.0]])
	radec = w.all_pix2world(pix, 0)
	ld.free()
	catalog = {'starid': np.array(starid + [77, 78]), 'tmag': np.array([9.5, 10.0, 10.5, 13.0, 13.5]), 'ra': radec[[0, 3, 4, 1, 2], 0], 'dec': radec[[0, 3, 4, 1, 2], 1]}
	targets = {'starid': np.array(starid), 'tmag': np.array([9.5, 10.0, 10.5]), 'ra': radec[[0, 3, 4], 0], 'dec': radec[[0, 3, 4], 1]}
	ctx.profile(True)
	ctx.profile_reset()
	(res,) = list(tessphot_tpfs(ctx, files, catalog, targets=targets))
	ctx.sync()
	report = ctx.profile_report()
	ctx.profile(False)
	assert _launches(report, 'world2pix') == 1, report
	for i, path in enumerate(files):
		(ld,) = tpf.load_tpfs(ctx, [path])
		pho = tessphot('aperture', starid[i], tpf.TpfStampSource(ld, catalog, targets=targets), str(tmp_path), datasource='tpf', ctx=ctx, version=VERSION)
		sumimage = None if pho._sumimage is None else np.array(pho._sumimage)
		ld.free()
		pho._details = {k: v for k, v in pho._details.items() if k != 'filepath_lightcurve'}   # (this batch wrote no files)
		_hold_result(res[i], pho, sumimage, res.sumimage(i), f'ra/dec file {i}')
	assert sum(res.status[i] in (STATUS.OK.value, STATUS.WARNING.value) for i in range(3)) >= 2
