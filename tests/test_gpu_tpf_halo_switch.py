# -*- coding: utf-8 -*-
"""
``tessphot_tpfs(..., method=)``: the method switch of ``tessphot(None, ...)`` and ``tessphot('halo', ...)`` for a batch of target pixel
files, against the per-file calls on the same device.  The six files are those of tests/halo_cubes_common.py (held to their conditions
on the oracle in tests/test_tpf_halo_switch_host.py): three ``Tmag <= 6`` stars with flux on the stamp edge -- one with two segments,
one with one, one whose second segment is degenerate --, a bright star inside its stamp and two faint ones, in groups of 11 x 11 x 70
(four files) and 9 x 13 x 70 (two).  Every result is held to the per-file one field by field: status, method, mask, every light-curve
column bit for bit (``flux_err`` to the bound of tests/test_gpu_halo_frames.py), the details key by key, the weight maps; the files
HDU by HDU, ``WEIGHTMAP`` included, as tests/test_gpu_lightcurve_files.py compares them.
"""
import gzip
import os
import numpy as np
import pytest
import halo_cubes_common as cc
from photometry_amd import tpf, tessphot, tessphot_tpfs, STATUS
from test_gpu_lightcurve_files import _hold_files

pytestmark = pytest.mark.gpu

VERSION = cc.VERSION
FLUX_ERR_RTOL = 4096 * 2.0**-53
SWITCHED = 'Automatically switched to Halo photometry'


def _bits_equal(a, b):
	a, b = np.asarray(a), np.asarray(b)
	return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view('uint8'), np.ascontiguousarray(b).view('uint8'))


def _per_file(ctx, made, method, out):
	"""The per-file call for every file: ``(pho, sum image)``."""
	res = []
	for path, starid in zip(made['files'], made['starid']):
		(ld,) = tpf.load_tpfs(ctx, [path])
		pho = tessphot(method, starid, tpf.TpfStampSource(ld, made['catalog'], targets=made['targets']), str(out), datasource='tpf', ctx=ctx, version=VERSION)
		res.append((pho, None if getattr(pho, '_sumimage', None) is None else np.array(pho._sumimage)))
		ld.free()
	return res


def _batch(ctx, made, out, **kw):
	chunks = list(tessphot_tpfs(ctx, made['files'], made['catalog'], targets=made['targets'], output_folder=None if out is None else str(out), version=VERSION, **kw))
	assert len(chunks) == 1
	return chunks[0]


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.fixture(scope='module')
def runs(ctx, tmp_path_factory):
	"""Every run of the module, once: the per-file calls and the batches, with Halo photometry on and off."""
	root = tmp_path_factory.mktemp('tpfhalo')
	made = cc.write_switch_files(root)
	ini = root / 'settings.ini'
	ini.write_text('[halo]\nenabled = true\n')
	folder = lambda name: tmp_path_factory.mktemp(name)
	r = {'made': made, 'folders': {}}

	def keep(name, per_file=None, **kw):
		r['folders'][name] = str(folder(name))
		r[name] = _per_file(ctx, made, per_file[0], r['folders'][name]) if per_file is not None else _batch(ctx, made, r['folders'][name], **kw)
	mp = pytest.MonkeyPatch()
	try:
		mp.delenv('TESSPHOT_SETTINGS', raising=False)
		keep('plugin_aperture', per_file=('aperture',))
		keep('plugin_none_off', per_file=(None,))
		keep('batch_none_off', method=None)
		mp.setenv('TESSPHOT_SETTINGS', str(ini))
		keep('plugin_none', per_file=(None,))
		keep('plugin_halo', per_file=('halo',))
		ctx.profile(True)
		ctx.profile_reset()
		keep('batch_none', method=None)
		ctx.sync()
		r['report'] = ctx.profile_report()
		ctx.profile(False)
		keep('batch_halo', method='halo')
		keep('batch_aperture', method='aperture')
		keep('batch_default')
		keep('batch_none_device', method=None, compress='device')
		keep('batch_none_table', method=None, compress='device', table='device')
	finally:
		mp.undo()
	return r


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
	"""``r`` (the batch's) against ``pho`` (the per-file call's), as tests/test_gpu_tpf_batch.py::_hold_result with the method and the
	weight maps: everything by its bits but ``flux_err`` of a Halo light curve, which is held to :data:`FLUX_ERR_RTOL`."""
	assert r.status == pho.status, (label, r.status, pho.status, r._details, pho._details)
	assert r.method == pho.method and r.starid == pho.starid, (label, r.method, pho.method)
	ok = pho.status in (STATUS.OK, STATUS.WARNING)
	if ok:
		assert list(r.lightcurve.keys()) == list(pho.lightcurve.keys()), label
	worst = 0.0
	if r.lightcurve is not None:
		for key in r.lightcurve.keys():
			if key == 'flux_err' and r.method == 'halo':
				ref = np.asarray(pho.lightcurve[key], dtype='float64')
				err = np.abs(r.lightcurve[key] - ref)
				worst = float(np.max(err / np.where(ref > 0, ref, 1.0)))
				print(f"{label}: worst relative flux_err difference {worst:.3e} (bound {FLUX_ERR_RTOL:.3e})")
				assert r.lightcurve[key].dtype == ref.dtype and np.all(err <= FLUX_ERR_RTOL * np.abs(ref)), (label, worst)
			else:
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
	if r.method == 'aperture':
		assert mine['stamp_resizes'] == 0 and r.halo_weightmap is None
	theirs_wm = getattr(pho, 'halo_weightmap', None) if pho.status == STATUS.OK and pho.method == 'halo' else None
	assert (r.halo_weightmap is None) == (theirs_wm is None), label
	if theirs_wm is not None:
		for key in ('initial_cadence', 'final_cadence', 'sat_pixels'):
			assert list(r.halo_weightmap[key]) == list(theirs_wm[key]), (label, key)
		assert len(r.halo_weightmap['weightmap']) == len(theirs_wm['weightmap'])
		for x, y in zip(r.halo_weightmap['weightmap'], theirs_wm['weightmap']):
			assert _bits_equal(x, y), label
	return worst


def _hold_folder(res, phos, out, plugin_out, label):
	"""The files of a batch against the per-file calls': a file for every OK / WARNING result and no other, every file HDU by HDU.
	(The per-file ``tessphot(None, ...)`` leaves the aperture run's file behind when the Halo run it switched to fails; the batch has
	written nothing yet when it switches.  The results name no file there, either of them.)"""
	wrote = [i for i in range(len(res)) if res.status[i] in (STATUS.OK.value, STATUS.WARNING.value)]
	assert sorted(os.listdir(out)) == sorted(os.path.basename(res.filepaths[i]) for i in wrote), label
	assert set(os.listdir(out)) <= set(os.listdir(plugin_out)), label
	for i in range(len(res)):
		if i in wrote:
			name = os.path.basename(res.filepaths[i])
			assert res[i]._details['filepath_lightcurve'] == phos[i][0]._details['filepath_lightcurve'] == name
			problems = _hold_files(os.path.join(out, name), os.path.join(plugin_out, name), res.sumimage(i), f'{label} file {i}')
			assert not problems, (label, i, problems)
		else:
			assert res.filepaths[i] is None and 'filepath_lightcurve' not in res[i]._details and 'filepath_lightcurve' not in phos[i][0]._details
	return wrote


def test_the_fixture_switches_exactly_the_intended_files(runs):
	from photometry_amd.tessphot import halo_switch_reason, _SWITCH_TEXT
	reasons = [halo_switch_reason(pho) for pho, _ in runs['plugin_aperture']]
	assert [i for i, why in enumerate(reasons) if why is not None] == list(cc.SWITCHING), reasons
	assert all(reasons[i] == _SWITCH_TEXT[2] for i in cc.SWITCHING)                        # the edge-flux reason
	for i, (pho, _) in enumerate(runs['plugin_aperture']):
		assert pho.status in (STATUS.OK, STATUS.WARNING), (i, pho.status, pho._details)
	tmag = [pho.target['tmag'] for pho, _ in runs['plugin_aperture']]
	assert sum(t <= 6 for t in tmag) == 4 and tmag[4] > 6 and tmag[5] > 6
	# what the per-file tessphot(None, ...) makes of them: two Halo light curves, one degenerate problem
	phos = [pho for pho, _ in runs['plugin_none']]
	assert [p.method for p in phos] == ['halo', 'halo', 'aperture', 'halo', 'aperture', 'aperture']
	assert phos[cc.DEGENERATE].status == STATUS.ERROR and 'ERROR: Halo optimization failed' in phos[cc.DEGENERATE]._details['errors']
	assert phos[0].status == STATUS.OK and phos[1].status == STATUS.OK
	assert len(phos[0].halo_weightmap['weightmap']) == 2 and len(phos[1].halo_weightmap['weightmap']) == 1


def test_method_none_equals_the_per_file_switch(runs):
	res, phos = runs['batch_none'], runs['plugin_none']
	assert sorted(res.halo_rows) == list(cc.SWITCHING)
	worst = 0.0
	for i in range(len(res)):
		pho, sumimage = phos[i]
		worst = max(worst, _hold_result(res[i], pho, sumimage, res.sumimage(i), f'method=None file {i}'))
		assert res.status[i] == pho.status.value
	print(f"method=None: worst relative flux_err difference {worst:.3e} (bound {FLUX_ERR_RTOL:.3e})")
	for i in cc.SWITCHING:
		r = res[i]
		assert r.method == 'halo' and SWITCHED in r._details['errors'] and r._details['edge_flux'] is not None
		assert _bits_equal(np.float64(r._details['edge_flux']), np.float64(runs['plugin_aperture'][i][0]._details['edge_flux']))   # the aperture run's
	for i in (0, 1):
		lc, ld = res[i].lightcurve, res.loaded[i]
		assert res[i].halo_weightmap is not None
		assert _bits_equal(lc['time'], ld.time) and _bits_equal(lc['pos_corr'], ld.pos_corr) and _bits_equal(lc['quality'], ld.quality)
		assert _bits_equal(lc['cadenceno'], ld.cadenceno) and lc['timecorr'].dtype == np.float64
	# one solver call for the chunk's group of 11 x 11 files, one for the 9 x 13 group; the cube kernels ran
	report = runs['report']
	assert report['tp_halo_cube_stat_kernel'][0] == 2 and report['tp_halo_cube_gather_kernel'][0] == 2 and report['tp_halo_cube_lightcurve_kernel'][0] == 2, report


def test_method_none_files(runs):
	wrote = _hold_folder(runs['batch_none'], runs['plugin_none'], runs['folders']['batch_none'], runs['folders']['plugin_none'], 'method=None')
	assert wrote == [0, 1, 2, 4, 5]
	from photometry_amd import fitsio
	for i in (0, 1):
		parts = fitsio.read(runs['batch_none'].filepaths[i])
		assert parts[0][0]['PHOTMET'] == 'halo' and parts[0][0]['NEXTEND'] == 4 and 'HALO_VER' in parts[0][0] and parts[-1][0]['EXTNAME'] == 'WEIGHTMAP'


def test_method_none_with_halo_off_records_the_request(runs):
	res, phos = runs['batch_none_off'], runs['plugin_none_off']
	assert not res.halo_rows
	for i in range(len(res)):
		pho, sumimage = phos[i]
		_hold_result(res[i], pho, sumimage, res.sumimage(i), f'Halo off, file {i}')
		assert res.status[i] == pho.status.value and res[i].method == 'aperture'
		requested = [e for e in res[i]._details.get('errors', []) if e.startswith('Halo switch requested (')]
		assert len(requested) == (1 if i in cc.SWITCHING else 0)
		if i in cc.SWITCHING:
			assert requested[0].endswith('but Halo photometry is not available: aperture result kept') and res[i]._details['errors'][-1] == requested[0]
			before = runs['plugin_aperture'][i][0].status
			assert res[i].status == (STATUS.WARNING if before == STATUS.OK else before)
	assert any(runs['plugin_aperture'][i][0].status == STATUS.OK for i in cc.SWITCHING)
	_hold_folder(res, phos, runs['folders']['batch_none_off'], runs['folders']['plugin_none_off'], 'Halo off')


def test_method_halo_equals_the_per_file_halo_run(runs):
	res, phos = runs['batch_halo'], runs['plugin_halo']
	for i in range(len(res)):
		pho, sumimage = phos[i]
		assert pho.method == 'halo'
		_hold_result(res[i], pho, sumimage, res.sumimage(i), f"method='halo' file {i}")
		assert SWITCHED not in res[i]._details.get('errors', [])
	assert [res[i].status for i in range(len(res))].count(STATUS.OK) >= 4 and res[cc.DEGENERATE].status == STATUS.ERROR
	assert sorted(res.halo_rows) == list(range(len(res)))
	_hold_folder(res, phos, runs['folders']['batch_halo'], runs['folders']['plugin_halo'], "method='halo'")


def test_method_halo_needs_halo_enabled(ctx, runs, monkeypatch):
	monkeypatch.delenv('TESSPHOT_SETTINGS', raising=False)
	made = runs['made']
	with pytest.raises(NotImplementedError, match=r'\[halo\] enabled = true'):
		list(tessphot_tpfs(ctx, made['files'], made['catalog'], targets=made['targets'], method='halo'))


def test_method_aperture_is_the_entry_without_the_keyword(runs):
	a, b = runs['batch_aperture'], runs['batch_default']
	assert not a.halo_rows and not b.halo_rows and not a.halo_requests
	for i in range(len(a)):
		x, y = a[i], b[i]
		assert x.method == y.method == 'aperture' and x.status == y.status and x.halo_weightmap is None
		assert (x.lightcurve is None) == (y.lightcurve is None)
		if x.lightcurve is not None:
			for key in y.lightcurve:
				assert _bits_equal(x.lightcurve[key], y.lightcurve[key]), (i, key)
			assert _bits_equal(x.final_phot_mask, y.final_phot_mask)
		assert set(x._details) == set(y._details)
		for key in y._details:
			assert _same_detail(key, x._details[key], y._details[key]), (i, key)
		pho, sumimage = runs['plugin_aperture'][i]
		assert x.status == pho.status
	fa, fb = runs['folders']['batch_aperture'], runs['folders']['batch_default']
	assert sorted(os.listdir(fa)) == sorted(os.listdir(fb)) and len(os.listdir(fa)) == 6
	for name in os.listdir(fa):
		with open(os.path.join(fa, name), 'rb') as f, open(os.path.join(fb, name), 'rb') as g:
			assert f.read() == g.read(), name


def test_an_invalid_method_raises_before_a_file_is_read(ctx, tmp_path):
	missing = str(tmp_path / 'no-such-file_tp.fits')
	with pytest.raises(ValueError, match=r"Invalid method: 'bogus'"):
		list(tessphot_tpfs(ctx, [missing], {}, method='bogus'))
	with pytest.raises(OSError):                                             # (a valid method gets as far as the file)
		list(tessphot_tpfs(ctx, [missing], {}, method=None))


@pytest.mark.parametrize('name', ('batch_none_device', 'batch_none_table'))
def test_device_compression_gives_the_same_bytes(runs, name):
	zl, dev = runs['folders']['batch_none'], runs['folders'][name]
	assert sorted(os.listdir(zl)) == sorted(os.listdir(dev)) and len(os.listdir(dev)) == 5
	assert [p and os.path.basename(p) for p in runs[name].filepaths] == [p and os.path.basename(p) for p in runs['batch_none'].filepaths]
	for fname in os.listdir(zl):
		with open(os.path.join(zl, fname), 'rb') as f, open(os.path.join(dev, fname), 'rb') as g:
			assert gzip.decompress(f.read()) == gzip.decompress(g.read()), fname
