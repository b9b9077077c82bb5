# -*- coding: utf-8 -*-
"""
``tessphot_tpfs(..., method='linpsf')`` against the per-file ``tessphot('linpsf', starid, TpfStampSource(loaded, catalog, prf=model), out,
datasource='tpf')`` on the same device.  Six files in one call (tests/tpf_linpsf_common.py): four of 11 x 11 x 70 -- one with two
non-finite ``TIME`` rows, which leaves its group on the device, one whose ``TICID`` is in no catalogue --, one of 9 x 13 x 70, one of
11 x 11 x 45; 1 to 4 fitted stars, a neighbour brighter than its target, NaN ``POS_CORR`` rows, a NaN pixel series, a NaN ``TIMECORR``
(positions through a lookup).  With ``[linpsf] flux_errors`` on every result is the per-file one: status, every light-curve column bit
for bit, ``PSF_CONT``, the details key by key, the errors, the files byte for byte after gunzip (``zlib``, ``compress='device'`` and
``table='device'``).  With it off every target ends in ERROR with the flux of the other run and no file.  A budget of one slot per slice
changes no bit, and the flux of two files is held to the oracle's LinPSF restatement on restated positions.
"""
import gzip
import os
import numpy as np
import pytest
import tpf_linpsf_common as lc
from photometry_amd import tpf, pipeline, tessphot, tessphot_tpfs, STATUS, psf as hpsf

pytestmark = pytest.mark.gpu

VERSION = lc.VERSION


def _bits_equal(a, b):
	a, b = np.asarray(a), np.asarray(b)
	return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view('uint8'), np.ascontiguousarray(b).view('uint8'))


def _last_lines(errors):
	return [str(e).strip().splitlines()[-1] for e in errors]


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.fixture(scope='module')
def runs(ctx, tmp_path_factory):
	"""Every run of the module, once.  ``TESSPHOT_SETTINGS`` is restored afterwards."""
	root = tmp_path_factory.mktemp('tpflinpsf')
	files, starid, catalog, prf = lc.write_files(root)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	ini = root / 'settings.ini'
	ini.write_text('[linpsf]\nflux_errors = true\n')
	r = {'files': files, 'starid': starid, 'catalog': catalog, 'prf': prf, 'model': model, 'folders': {}}

	def per_file(name):
		out = r['folders'][name] = str(tmp_path_factory.mktemp(name))
		res = []
		for path, sid in zip(files, starid):
			(ld,) = tpf.load_tpfs(ctx, [path])
			pho = tessphot('linpsf', sid, tpf.TpfStampSource(ld, catalog, prf=model), out, datasource='tpf', ctx=ctx, version=VERSION)
			res.append((pho, None if getattr(pho, '_sumimage', None) is None else np.array(pho._sumimage)))
			ld.free()
		r[name] = res

	def batch(name, **kw):
		out = r['folders'][name] = str(tmp_path_factory.mktemp(name))
		chunks = list(tessphot_tpfs(ctx, files, catalog, output_folder=out, version=VERSION, method='linpsf', prf=model, **kw))
		assert len(chunks) == 1
		r[name] = chunks[0]
	old = os.environ.get('TESSPHOT_SETTINGS')
	try:
		os.environ.pop('TESSPHOT_SETTINGS', None)
		batch('batch_off')
		per_file('plugin_off')
		os.environ['TESSPHOT_SETTINGS'] = str(ini)
		per_file('plugin_on')
		ctx.profile(True)
		ctx.profile_reset()
		batch('batch_on')
		ctx.sync()
		r['report'] = ctx.profile_report()
		ctx.profile(False)
		batch('batch_device', compress='device')
		batch('batch_table', compress='device', table='device')
	finally:
		if old is None:
			os.environ.pop('TESSPHOT_SETTINGS', None)
		else:
			os.environ['TESSPHOT_SETTINGS'] = old
	return r


def _same_detail(key, a, b):
	if key == 'errors':
		return _last_lines(a) == _last_lines(b)
	if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
		return _bits_equal(np.asarray(a, dtype='float64'), np.asarray(b, dtype='float64'))
	if isinstance(a, float) or isinstance(b, float):
		return _bits_equal(np.float64(a), np.float64(b))
	return type(a) == type(b) and a == b


def _hold_result(r, pho, label):
	"""``r`` (the batch's) against ``pho`` (the per-file call's): everything by its bits."""
	assert r.status == pho.status, (label, r.status, pho.status, r._details, pho._details)
	assert r.method == pho.method == 'linpsf' and r.starid == pho.starid, label
	assert r.final_phot_mask is None and pho.final_phot_mask is None and r.halo_weightmap is None
	assert list(r.lightcurve.keys()) == list(pho.lightcurve.keys()), label
	for key in pho.lightcurve.keys():
		assert _bits_equal(r.lightcurve[key], pho.lightcurve[key]), (label, key)
	mine, theirs = dict(r._details), dict(pho._details)
	assert set(mine) == set(theirs), (label, sorted(mine), sorted(theirs))
	for key, value in theirs.items():
		assert _same_detail(key, mine[key], value), (label, key, mine[key], value)
	assert list(r.additional_headers) == list(pho.additional_headers), label
	for key, (value, comment) in pho.additional_headers.items():
		assert r.additional_headers[key][1] == comment and _same_detail(key, r.additional_headers[key][0], value), (label, key)


def test_the_fixture_is_what_the_module_says(runs):
	res, phos = runs['batch_on'], [p for p, _ in runs['plugin_on']]
	shapes = sorted(tuple(np.shape(ld.aperture)) + (len(ld.time),) for ld in res.loaded)
	assert shapes == [(9, 13, 70), (11, 11, 45), (11, 11, 68), (11, 11, 70), (11, 11, 70), (11, 11, 70)]
	fitted = sorted(res.linpsf[p][j]['n_stars'] for p, j in res._linpsf_where.values())
	assert fitted[0] == 1 and fitted[-1] == 4 and len(fitted) == 5
	assert np.isnan(res.loaded[lc.NAN_POS_CORR].pos_corr).any() and np.isnan(res.loaded[lc.NAN_TIMECORR].timecorr).sum() == 1
	assert tpf.jitter_lookup(res.loaded[lc.NAN_TIMECORR].time, res.loaded[lc.NAN_TIMECORR].timecorr) is not None
	print([(p.status, p._details.get('errors')) for p in phos])
	assert STATUS.WARNING in [p.status for p in phos] and STATUS.OK in [p.status for p in phos]
	assert 'High contamination' in phos[4]._details['errors']            # (the brighter neighbour)


def test_flux_errors_on_equals_the_per_file_run(runs):
	res, phos = runs['batch_on'], runs['plugin_on']
	assert len(res) == 6
	for i in range(6):
		pho, sumimage = phos[i]
		if i == lc.LOST:
			# the per-file call never gets a photometry object: the error and nothing else
			r = res[i]
			assert pho.method == 'error' and r.status == pho.status == STATUS.ERROR and r.lightcurve is None and r.final_phot_mask is None
			assert _last_lines(r._details['errors']) == _last_lines(pho._details['errors']) == [f'RuntimeError: Star could not be found in catalog: {runs["starid"][i]}']
			assert set(r._details) == {'errors'} and res.filepaths[i] is None
			continue
		_hold_result(res[i], pho, f'file {i}')
		assert res.status[i] == pho.status.value
		assert pho.status in (STATUS.OK, STATUS.WARNING), (i, pho._details)
		assert res[i].additional_headers['PSF_FERR'][0] is True and np.isfinite(res[i].lightcurve['flux_err']).any()
		assert _bits_equal(res.sumimage(i), sumimage), i
		ld = res.loaded[i]
		assert _bits_equal(res[i].lightcurve['pos_corr'], ld.pos_corr) and _bits_equal(res[i].lightcurve['time'], ld.time)
	# one pass per group: two position launches per group (11 x 11 x 70, 11 x 11 x 68, 9 x 13 x 70, 11 x 11 x 45) and two for the lookup
	report = runs['report']
	assert report['tp_star_positions_targets_kernel'][0] == 10, report
	# (the error pass launches once per class of star counts in a slice, at least once per group)
	assert report['tp_linpsf_err_kernel'][0] >= 4 and report['tp_diagnostics_kernel'][0] == 4 and report['tp_sumimage_kernel'][0] == 4, report
	assert 'tp_k2p2_kernel' not in report and 'tp_aperture_fused_kernel' not in report, report


def test_flux_errors_off_is_the_reference(runs):
	off, on, phos = runs['batch_off'], runs['batch_on'], runs['plugin_off']
	assert os.listdir(runs['folders']['batch_off']) == [] and off.filepaths == [None] * 6
	for i in range(6):
		r = off[i]
		assert r.status == STATUS.ERROR and off.status[i] == STATUS.ERROR.value
		if i == lc.LOST:
			continue
		assert np.all(np.isnan(r.lightcurve['flux_err']))
		assert _bits_equal(r.lightcurve['flux'], on[i].lightcurve['flux']), i
		assert _last_lines(r._details['errors'])[-1] == 'ValueError: Final lightcurve errors are all NaNs'
		assert 'PSF_FERR' not in r.additional_headers and 'filepath_lightcurve' not in r._details
		_hold_result(r, phos[i][0], f'errors off, file {i}')


def test_files_equal_the_per_file_files(runs):
	res, phos = runs['batch_on'], runs['plugin_on']
	out, plugin_out = runs['folders']['batch_on'], runs['folders']['plugin_on']
	wrote = [i for i in range(6) if res.status[i] in (STATUS.OK.value, STATUS.WARNING.value)]
	assert wrote == [1, 2, 3, 4, 5]
	assert sorted(os.listdir(out)) == sorted(os.path.basename(res.filepaths[i]) for i in wrote) == sorted(os.listdir(plugin_out))
	from photometry_amd import fitsio
	for i in wrote:
		name = os.path.basename(res.filepaths[i])
		assert res[i]._details['filepath_lightcurve'] == phos[i][0]._details['filepath_lightcurve'] == name
		with open(os.path.join(out, name), 'rb') as f, open(os.path.join(plugin_out, name), 'rb') as g:
			assert gzip.decompress(f.read()) == gzip.decompress(g.read()), name
		primary = fitsio.read(os.path.join(out, name))[0][0]
		assert primary['PHOTMET'] == 'linpsf' and 'PSF_CONT' in primary and 'PSF_FERR' in primary and 'KP_THRES' not in primary


@pytest.mark.parametrize('name', ('batch_device', 'batch_table'))
def test_device_compression_gives_the_same_bytes(runs, name):
	zl, dev = runs['folders']['batch_on'], runs['folders'][name]
	assert sorted(os.listdir(zl)) == sorted(os.listdir(dev)) and len(os.listdir(dev)) == 5
	assert [p and os.path.basename(p) for p in runs[name].filepaths] == [p and os.path.basename(p) for p in runs['batch_on'].filepaths]
	for fname in os.listdir(zl):
		with open(os.path.join(zl, fname), 'rb') as f, open(os.path.join(dev, fname), 'rb') as g:
			assert gzip.decompress(f.read()) == gzip.decompress(g.read()), fname


def _group_inputs(ctx, runs, want):
	"""The group of ``load_tpf_groups`` with shape ``want`` and what ``pipeline.linpsf_tpfs`` takes for its slots."""
	groups, index = tpf.load_tpf_groups(ctx, runs['files'])
	g = [grp.shape for grp in groups].index(want)
	grp = groups[g]
	files_of = [i for s in range(len(grp)) for i, (gg, ss) in enumerate(index) if (gg, ss) == (g, s)]
	cats = [pipeline._catalog_of_stamp(runs['catalog'], grp.loaded[s].max_stamp) for s in range(len(grp))]
	return groups, grp, files_of, cats


def test_a_slice_boundary_changes_no_bit(ctx, runs):
	groups, grp, files_of, cats = _group_inputs(ctx, runs, (11, 11, 70))
	try:
		assert files_of[0] == lc.LOST and len(grp) == 3                 # the file without a target sits in slot 0: the fit starts behind it
		slots = [1, 2]
		starid = [runs['starid'][files_of[s]] for s in slots]
		args = (ctx, grp, slots, [cats[s] for s in slots], np.zeros((2, 3)), starid, runs['model'])
		whole = pipeline.linpsf_tpfs(*args, flux_errors=True)
		ctx.profile(True)
		ctx.profile_reset()
		sliced = pipeline.linpsf_tpfs(*args, flux_errors=True, budget_bytes=1)
		ctx.sync()
		report = ctx.profile_report()
		ctx.profile(False)
		assert report['tp_star_positions_targets_kernel'][0] == 4, report     # one slot per slice: two launches each
		for key in ('flux', 'flux_err', 'contamination', 'status', 'stamp'):
			assert _bits_equal(getattr(whole, key), getattr(sliced, key)), key
		assert whole.errors == sliced.errors and np.isfinite(whole.flux).any()
		on = runs['batch_on']
		for j, s in enumerate(slots):
			assert _bits_equal(whole.flux[j], on[files_of[s]].lightcurve['flux']) and _bits_equal(whole.flux_err[j], on[files_of[s]].lightcurve['flux_err'])
		# the file without its target handed in all the same: an error of its own, the others untouched
		three = pipeline.linpsf_tpfs(ctx, grp, [0, 1, 2], cats, np.zeros((3, 3)), [runs['starid'][i] for i in files_of], runs['model'], flux_errors=True)
		assert three.status[0] == STATUS.ERROR.value and three.errors[0] == ['ValueError: main target missing from its catalog'] and np.all(np.isnan(three.flux[0]))
		assert _bits_equal(three.flux[1:], whole.flux) and _bits_equal(three.flux_err[1:], whole.flux_err)
	finally:
		for g in groups:
			g.free()


@pytest.mark.parametrize('kind', ['same_knots', 'other_knots'])
def test_a_model_per_camera_and_ccd(ctx, runs, kind, monkeypatch, tmp_path):
	"""``prf`` as a mapping: files 2 (camera 1) and 3 (camera 2) lie in one group and get the coefficients of their own model -- in one
	pass when the models share their knots, in a pass each when they do not -- and every file the flux of the per-file plugin with its model."""
	from photometry_amd import simulate
	from photometry_amd.plugins import LinPSFPhotometry
	monkeypatch.delenv('TESSPHOT_SETTINGS', raising=False)
	other = simulate.synthetic_prf(seed=3) if kind == 'same_knots' else simulate.synthetic_prf(seed=3, halfwidth=5.5)
	second = hpsf.PRFModel(other['values'], other['ccdColumn'], other['ccdRow'], other['prfColumn'], other['prfRow'])
	first = runs['model']
	assert np.array_equal(first.tx, second.tx) == (kind == 'same_knots')
	models = {(1, 2): first, (2, 2): second}
	(res,) = list(tessphot_tpfs(ctx, runs['files'], runs['catalog'], method='linpsf', prf=models))
	differs = 0
	for i in range(1, 6):
		ld = res.loaded[i]
		(one,) = tpf.load_tpfs(ctx, [runs['files'][i]])
		with LinPSFPhotometry(runs['starid'][i], tpf.TpfStampSource(one, runs['catalog'], prf=models[(ld.camera, ld.ccd)]), str(tmp_path), datasource='tpf', ctx=ctx) as pho:
			pho.do_photometry()
			assert _bits_equal(res[i].lightcurve['flux'], pho.lightcurve['flux']), (kind, i)
			assert _bits_equal(np.float64(res[i].additional_headers['PSF_CONT'][0]), np.float64(pho.additional_headers['PSF_CONT'][0])), (kind, i)
		one.free()
		differs += not _bits_equal(res[i].lightcurve['flux'], runs['batch_off'][i].lightcurve['flux'])
	assert differs == sum(res.loaded[i].camera == 2 for i in range(1, 6)) == 3     # (the second model is another PRF)


@pytest.mark.parametrize('i', [1, 4])
def test_flux_against_the_oracle(runs, i):
	"""Independence from the device's side: the oracle's LinPSF on the file's pixels with the positions restated in numpy, at the tolerance
	tests/test_gpu_linpsf.py holds the fit to."""
	from oracle import psf as opsf, linpsf as olin
	res, prf = runs['batch_on'], runs['prf']
	ld = res.loaded[i]
	rec_cat = pipeline._catalog_of_stamp(runs['catalog'], ld.max_stamp)
	T = len(ld.time)
	n = len(rec_cat['starid'])
	assert tpf.jitter_lookup(ld.time, ld.timecorr) is None
	positions = np.empty((T, n, 2))
	positions[:, :, 0] = lc.positions_numpy(rec_cat['row_stamp'], np.zeros(n, dtype='int64'), ld.pos_corr[None, :, 1], T).T
	positions[:, :, 1] = lc.positions_numpy(rec_cat['column_stamp'], np.zeros(n, dtype='int64'), ld.pos_corr[None, :, 0], T).T
	pho = runs['plugin_on'][i][0]
	images = pho.images_cube
	p = opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(ld.max_stamp))
	k = int(np.flatnonzero(rec_cat['starid'] == runs['starid'][i])[0])
	ref = olin.do_photometry(images, p, rec_cat, runs['starid'][i], positions, tuple(ld.max_stamp), float(rec_cat['row'][k]), float(rec_cat['column'][k]),
		np.asarray(ld.aperture))
	flux = res[i].lightcurve['flux']
	scale = np.nanmax(np.abs(ref['flux']))
	worst = float(np.nanmax(np.abs(flux - ref['flux']) / (1e-8 * np.abs(ref['flux']) + 1e-9 * scale)))
	print(f'file {i}: worst flux difference against the oracle {worst:.3e} of the bound (rtol 1e-8, atol 1e-9 * scale)')
	np.testing.assert_allclose(flux, ref['flux'], rtol=1e-8, atol=1e-9 * scale)
	np.testing.assert_allclose(res[i].additional_headers['PSF_CONT'][0], ref['contamination'], rtol=1e-7, atol=1e-11)


def test_linpsf_gets_as_far_as_the_missing_file(ctx, tmp_path):
	missing = str(tmp_path / 'no-such-file_tp.fits')
	with pytest.raises(ValueError, match=r"Invalid method: 'psf'"):
		list(tessphot_tpfs(ctx, [missing], {}, method='psf'))
	with pytest.raises(OSError):
		list(tessphot_tpfs(ctx, [missing], {}, method='linpsf'))
