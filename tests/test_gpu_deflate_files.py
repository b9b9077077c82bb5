# -*- coding: utf-8 -*-
"""
Light-curve files compressed on the device (``compress='device'``; photometry_amd/lcfile.py, photometry_amd/deflate.py): the frames
entry over the region of tests/test_gpu_lightcurve_files.py and ``tessphot_tpfs`` over three small target pixel files written as
tests/test_gpu_tpf_batch.py writes its own, each once with ``compress='zlib'`` and once with ``'device'``.  The two runs give the same
file names and, decompressed, the same bytes; ``fitsio.read`` finds CHECKSUM / DATASUM in order; a second ``'device'`` run writes the
same file bytes; the default run launches no deflate kernel, the ``'device'`` run one per batch.
"""
import gzip
import os
import numpy as np
import pytest
from test_gpu_lightcurve_files import _region
from test_gpu_tpf_batch import _write

pytestmark = pytest.mark.gpu

VERSION = 6


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _launches(report, word):
	return sum(n for name, (n, _ms) in report.items() if word in name)


def _profiled(ctx, run):
	ctx.profile(True)
	ctx.profile_reset()
	out = run()
	ctx.sync()
	report = ctx.profile_report()
	ctx.profile(False)
	return out, report


def _same_files(a, b, c, n_files):
	"""Folders ``a`` (zlib), ``b`` and ``c`` (device, two runs)."""
	from photometry_amd import fitsio
	names = sorted(os.listdir(a))
	assert names == sorted(os.listdir(b)) == sorted(os.listdir(c)) and len(names) == n_files
	for name in names:
		with open(os.path.join(a, name), 'rb') as fh:
			zl = fh.read()
		with open(os.path.join(b, name), 'rb') as fh:
			dev = fh.read()
		with open(os.path.join(c, name), 'rb') as fh:
			dev2 = fh.read()
		assert gzip.decompress(dev) == gzip.decompress(zl), name                      # byte for byte
		assert dev == dev2, name                                                      # a second run: identical file bytes
		assert dev[:10] == b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff' and dev != zl
		for header, _data in fitsio.read(os.path.join(b, name)):
			assert header['__checksum_ok__'] is True and header['__datasum_ok__'] is True, (name, header.get('EXTNAME'))


def test_frames_entry(ctx, tmp_path):
	from photometry_amd import pipeline, tessphot_frames, STATUS
	from photometry_amd.lcfile import FileInfo
	frames, row0, col0, time, quality, cat, targets = _region()
	R, C, T = frames['images'].shape
	rng = np.random.default_rng(8)
	fr = {k: np.ascontiguousarray(np.moveaxis(v, 2, 0)) for k, v in frames.items()}
	flags = rng.integers(0, 8, (T, R, C)).astype('uint8')
	stack = pipeline.FrameStack(ctx, dict(fr, pixel_flags=flags), row0, col0)
	info = FileInfo(14, 2, 3)
	timecorr = 1e-3 * rng.normal(size=T)

	def run(folder, **kw):
		return tessphot_frames(ctx, stack, targets, cat, time, quality, timecorr=timecorr, cadenceno=np.arange(T), output_folder=str(tmp_path / folder), fileinfo=info,
			version=VERSION, **kw)
	plain, report = _profiled(ctx, lambda: run('zlib'))
	assert _launches(report, 'deflate') == 0, report                                   # the default launches no new kernel
	explicit = run('zlib2', compress='zlib')
	dev, report = _profiled(ctx, lambda: run('device', compress='device'))
	assert report['tp_deflate_kernel'][0] == 1 and report['tp_deflate_scan_kernel'][0] == 1 and report['tp_deflate_pack_kernel'][0] == 1, report
	dev2 = run('device2', compress='device')
	n_files = int(np.sum((plain.status == STATUS.OK.value) | (plain.status == STATUS.WARNING.value)))
	assert n_files >= 5
	assert [p and os.path.basename(p) for p in dev.filepaths] == [p and os.path.basename(p) for p in plain.filepaths]
	_same_files(tmp_path / 'zlib', tmp_path / 'device', tmp_path / 'device2', n_files)
	for name in os.listdir(tmp_path / 'zlib'):                                        # compress='zlib' is the default, to the compressed byte
		with open(tmp_path / 'zlib' / name, 'rb') as fa, open(tmp_path / 'zlib2' / name, 'rb') as fb:
			assert fa.read()[10:] == fb.read()[10:]                                    # (behind gzip's own header with its MTIME)
	assert dev2.filepaths is not None and explicit.filepaths is not None
	with pytest.raises(ValueError, match='compress'):
		run('nope', compress='nope')
	with pytest.raises(ValueError, match='compress'):
		plain.save_lightcurves(str(tmp_path / 'nope2'), info, time, quality, VERSION, compress='gzip')
	# the timings of the device path
	from photometry_amd import lcfile
	timings = {}
	lcfile.save_lightcurves(dev, stack, str(tmp_path / 'device3'), info, time, quality, VERSION, timecorr=timecorr, cadenceno=np.arange(T), targets=targets,
		compress='device', compresslevel=1, timings=timings, workers=1)
	parts = timings.pop('gzip_parts')
	assert set(timings) == {'quality', 'build', 'gzip', 'write'} and all(v > 0 for v in timings.values())
	assert set(parts) == {'stage', 'upload_and_kernels', 'download', 'members'} and sum(parts.values()) <= timings['gzip']
	_same_files(tmp_path / 'zlib', tmp_path / 'device', tmp_path / 'device3', n_files)


def test_tessphot_tpfs(ctx, tmp_path):
	from photometry_amd import simulate, tessphot_tpfs
	root = tmp_path / 'tpfs'
	root.mkdir()
	rng = np.random.default_rng(62)
	s = simulate.make_scene(3, 70, 11, 11, seed=12, cadence_s=120.0)
	simulate.fill_cubes(s, nan_fraction=0.0)
	made = [_write(root, s, i, rng) for i in range(3)]
	files = [m[0] for m in made]
	cat = {k: s.catalog[k] for k in ('starid', 'tmag', 'row', 'column')}
	targets = {'starid': s.target_starid, 'tmag': s.target_tmag, 'row': s.target_pos_row, 'column': s.target_pos_column}

	def run(folder, **kw):
		return list(tessphot_tpfs(ctx, files, cat, targets=targets, output_folder=str(tmp_path / folder), version=VERSION, **kw))
	(plain,), report = _profiled(ctx, lambda: run('zlib'))
	assert _launches(report, 'deflate') == 0, report
	(dev,), report = _profiled(ctx, lambda: run('device', compress='device'))
	assert report['tp_deflate_kernel'][0] == 1, report
	(dev2,) = run('device2', compress='device', workers=1)
	n_files = sum(p is not None for p in plain.filepaths)
	assert n_files == 3
	assert [os.path.basename(p) for p in dev.filepaths] == [os.path.basename(p) for p in plain.filepaths]
	_same_files(tmp_path / 'zlib', tmp_path / 'device', tmp_path / 'device2', n_files)
	with pytest.raises(ValueError, match='compress'):
		run('nope', compress='nope')
	assert not os.path.exists(tmp_path / 'nope')
