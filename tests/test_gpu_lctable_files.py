# -*- coding: utf-8 -*-
"""
Light-curve files whose ``LIGHTCURVE`` table the device writes (``table='device'``: ``tp_lc_table_pack`` straight into the encoder's
input, DATASUM formed on the device, photometry_amd/lcfile.py) against the files of ``compress='device'`` alone and of the default
path: the same file names and, because the encoder's output depends on its input alone, the **same file bytes** as ``compress='device'``;
decompressed, the bytes of the ``compress='zlib'`` files; every ``CHECKSUM`` and ``DATASUM`` in order.  The frames entry runs over the
region of tests/test_gpu_lightcurve_files.py (pixel flags, a movement kernel), ``tessphot_tpfs`` over three small target pixel files
written as tests/test_gpu_tpf_batch.py writes its own, one of another length, so that two pack launches occur.  No tolerance anywhere.
"""
import gzip
import os
import numpy as np
import pytest
from test_gpu_lightcurve_files import _region
from test_gpu_tpf_batch import _write

pytestmark = pytest.mark.gpu

VERSION = 6
KERNELS = ('tp_lc_table_pack_kernel', 'tp_lc_table_fold_kernel', 'tp_lc_place_kernel')


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _files(folder):
	return {name: open(os.path.join(folder, name), 'rb').read() for name in sorted(os.listdir(folder))}


def _hold(zlib_dir, device_dir, table_dir):
	"""The three folders by the rule of the module's docstring; returns the number of files."""
	from photometry_amd import fitsio
	z, d, t = _files(zlib_dir), _files(device_dir), _files(table_dir)
	assert list(z) == list(d) == list(t) and len(t) > 0
	for name in t:
		assert t[name] == d[name], name                                       # the same file bytes
		assert gzip.decompress(t[name]) == gzip.decompress(z[name]), name     # the default path's content
		hdus = fitsio.read(os.path.join(table_dir, name))
		assert [h.get('EXTNAME') for h, _ in hdus][:4] == ['PRIMARY', 'LIGHTCURVE', 'SUMIMAGE', 'APERTURE']
		for header, _data in hdus:
			assert header['__checksum_ok__'] is True and header['__datasum_ok__'] is True, (name, header.get('EXTNAME'))
	return len(t)


def _profiled(ctx, run):
	ctx.profile(True)
	ctx.profile_reset()
	try:
		out = run()
		ctx.sync()
		return out, ctx.profile_report()
	finally:
		ctx.profile(False)


@pytest.fixture(scope='module')
def frames_runs(ctx, tmp_path_factory):
	"""The region through ``tessphot_frames`` three times -- default, ``compress='device'``, and with ``table='device'`` --, each under the profile."""
	from photometry_amd import pipeline, tessphot_frames
	from photometry_amd.lcfile import FileInfo
	from photometry_amd.motion import MovementKernel
	root = tmp_path_factory.mktemp('lctable_frames')
	frames, row0, col0, time, quality, cat, targets = _region()
	R, C, T = frames['images'].shape
	rng = np.random.default_rng(8)
	fr = {k: np.ascontiguousarray(np.moveaxis(v, 2, 0)) for k, v in frames.items()}
	flags = rng.integers(0, 8, (T, R, C)).astype('uint8')                     # bit 4 scattered: QUALITY rows that differ between the targets
	flags[rng.random(flags.shape) < 0.995] &= 3
	timecorr = 1e-3 * rng.normal(size=T)
	mk = MovementKernel('translation')
	mk.load_series(time - timecorr, 0.05 * rng.normal(size=(T, 2)))
	stack = pipeline.FrameStack(ctx, dict(fr, pixel_flags=flags, backgrounds_pixels_used=rng.random((R, C)) < 0.7), row0, col0)
	info = FileInfo(14, 2, 3, header={'DATA_REL': 20, 'CRMITEN': True, 'CRBLKSZ': 10, 'CRSPOC': False})
	out = {}
	for key, how in (('zlib', {}), ('device', dict(compress='device')), ('table', dict(compress='device', table='device'))):
		folder = str(root / key)
		res, report = _profiled(ctx, lambda: tessphot_frames(ctx, stack, targets, cat, time, quality, timecorr=timecorr, cadenceno=np.arange(T) + 4700, movement=mk,
			output_folder=folder, fileinfo=info, version=VERSION, **how))
		out[key] = (folder, res, report)
	out['call'] = dict(stack=stack, info=info, time=time, quality=quality, timecorr=timecorr, T=T, root=root)
	return out


def test_frames_entry_writes_the_same_files(frames_runs):
	n = _hold(*(frames_runs[k][0] for k in ('zlib', 'device', 'table')))
	res = frames_runs['table'][1]
	assert n == sum(p is not None for p in res.filepaths) >= 5
	assert [p and os.path.basename(p) for p in res.filepaths] == [p and os.path.basename(p) for p in frames_runs['device'][1].filepaths]
	assert res.pos_corr is not None and np.any(res.pos_corr != 0)
	# the QUALITY column is not all zero somewhere: the flag rows went through the pack
	from photometry_amd import fitsio
	assert any(fitsio.read(p)[1][1]['QUALITY'].any() for p in res.filepaths if p is not None)


def test_frames_entry_launch_counts(frames_runs):
	for key in ('zlib', 'device'):
		assert not [k for k in frames_runs[key][2] if k.startswith('tp_lc_')], key
	report = frames_runs['table'][2]
	assert [report[k][0] for k in KERNELS] == [1, 1, 1]                           # time is shared: one pack for the batch, one fold, one place
	print('pack kernel:', report['tp_lc_table_pack_kernel'])


def test_results_in_hand_with_nan_times(ctx, frames_runs):
	"""``BatchResults.save_lightcurves`` on results in hand, first, a middle and the last ``time`` NaN: the rows are dropped from every
	column on the device as on the host."""
	from photometry_amd import fitsio
	call, res = frames_runs['call'], frames_runs['zlib'][1]
	time = call['time'].copy()
	time[[0, 11, call['T'] - 1]] = np.nan
	folders = {}
	for key, how in (('zlib', {}), ('device', dict(compress='device')), ('table', dict(compress='device', table='device'))):
		folders[key] = str(call['root'] / ('nan_' + key))
		res.save_lightcurves(folders[key], call['info'], time, call['quality'], VERSION, timecorr=call['timecorr'], cadenceno=np.arange(call['T']) + 4700, **how)
	assert _hold(folders['zlib'], folders['device'], folders['table']) >= 5
	name = sorted(os.listdir(folders['table']))[0]
	header, tab = fitsio.read(os.path.join(folders['table'], name))[1]
	assert header['NAXIS2'] == call['T'] - 3 and np.array_equal(tab['TIME'], time[np.isfinite(time)]) and np.array_equal(tab['CADENCENO'], np.delete(np.arange(call['T']) + 4700, [0, 11, call['T'] - 1]))


def test_table_device_needs_compress_device(ctx, frames_runs, tmp_path):
	from photometry_amd import tessphot_frames, tessphot_frames_pipelined, tessphot_tpfs, lcfile
	call, res = frames_runs['call'], frames_runs['zlib'][1]
	with pytest.raises(ValueError, match="table='device' needs compress='device'"):
		res.save_lightcurves(str(tmp_path / 'a'), call['info'], call['time'], call['quality'], VERSION, table='device')
	with pytest.raises(ValueError, match="table='device' needs compress='device'"):
		res.save_lightcurves(str(tmp_path / 'a'), call['info'], call['time'], call['quality'], VERSION, compress='zlib', table='device')
	with pytest.raises(ValueError, match='table must be one of'):
		res.save_lightcurves(str(tmp_path / 'a'), call['info'], call['time'], call['quality'], VERSION, compress='device', table='gpu')
	with pytest.raises(ValueError, match="table='device' needs compress='device'"):
		tessphot_frames(ctx, call['stack'], res.targets, None, call['time'], call['quality'], table='device')
	with pytest.raises(ValueError, match="table='device' needs compress='device'"):
		list(tessphot_frames_pipelined(ctx, call['stack'], [res.targets], None, call['time'], call['quality'], table='device'))
	with pytest.raises(ValueError, match="table='device' needs compress='device'"):
		list(tessphot_tpfs(ctx, ['nothing.fits'], None, table='device', compress='zlib'))
	assert not os.path.exists(str(tmp_path / 'a')) and lcfile.TABLE == ('host', 'device')


@pytest.fixture(scope='module')
def tpf_runs(ctx, tmp_path_factory):
	"""Three target pixel files, the third of another length, through ``tessphot_tpfs`` three times."""
	from photometry_amd import simulate, tessphot_tpfs
	root = tmp_path_factory.mktemp('lctable_tpfs')
	rng = np.random.default_rng(62)
	a = simulate.make_scene(2, 70, 11, 11, seed=12, cadence_s=120.0)
	simulate.fill_cubes(a, nan_fraction=0.0)
	b = simulate.make_scene(1, 45, 11, 11, seed=13, cadence_s=120.0)
	simulate.fill_cubes(b, nan_fraction=0.0)
	flagged = np.zeros(70, dtype='int32')
	flagged[[3, 20, 60]] = [1, 8, 4096]
	made = [_write(root, a, 0, rng, bad_times=(33, 34)), _write(root, a, 1, rng, quality=flagged, bad_times=(33, 34)), _write(root, b, 0, rng, starid_offset=1000)]
	cat = {k: np.concatenate((a.catalog[k], b.catalog[k])) for k in ('starid', 'tmag', 'row', 'column')}
	cat['starid'] = np.concatenate((a.catalog['starid'], b.catalog['starid'] + 1000))
	targets = {'starid': np.concatenate((a.target_starid, b.target_starid + 1000)), 'tmag': np.concatenate((a.target_tmag, b.target_tmag)),
		'row': np.concatenate((a.target_pos_row, b.target_pos_row)), 'column': np.concatenate((a.target_pos_column, b.target_pos_column))}
	files = [m[0] for m in made]
	out = {}
	for key, how in (('zlib', {}), ('device', dict(compress='device')), ('table', dict(compress='device', table='device'))):
		folder = str(root / key)
		chunks, report = _profiled(ctx, lambda: list(tessphot_tpfs(ctx, files, cat, targets=targets, output_folder=folder, version=VERSION, **how)))
		assert len(chunks) == 1
		out[key] = (folder, chunks[0], report)
	return out


def test_tpf_entry_writes_the_same_files(tpf_runs):
	from photometry_amd import fitsio
	assert _hold(*(tpf_runs[k][0] for k in ('zlib', 'device', 'table'))) == 3
	res = tpf_runs['table'][1]
	assert all(p is not None for p in res.filepaths)
	rows = sorted(fitsio.read(p)[1][0]['NAXIS2'] for p in res.filepaths)
	assert rows == [45, 68, 68]                                                    # two lengths, the rows without a finite time dropped


def test_tpf_entry_launch_counts(tpf_runs):
	for key in ('zlib', 'device'):
		assert not [k for k in tpf_runs[key][2] if k.startswith('tp_lc_')], key
	report = tpf_runs['table'][2]
	assert [report[k][0] for k in KERNELS] == [2, 2, 1]                           # one pack (and fold) per (T, kept rows) set, one place for the window
