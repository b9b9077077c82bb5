# -*- coding: utf-8 -*-
"""
The light-curve files of the batched frames entry (``tessphot_frames(..., output_folder=, fileinfo=, version=)``;
photometry_amd/lcfile.py, the ``QUALITY`` column from csrc/stampflags.hip) against the files the per-target plugin writes for the same
targets over a ``MemoryStampSource`` of the same frames: decompressed, byte for byte, but for the primary header's ``DATE`` and
``CHECKSUM`` cards, which are compared only when both ``DATE`` values agree (the day of writing).

``SUMIMAGE`` is held to equality as well.  The batch crops the region's sum image (float64 sums in cadence order), the plugin sums its
own cube pairwise, and two float64 summation orders of the same ``T`` float32 terms may differ by ``2 (T - 1) 2^-53 mean_t |x|`` per
pixel of the mean -- but on the MI355X every pixel of every file came out bit-equal: a sum of 24 values of 24 significant bits is exact
in float64 unless the values of one pixel span more than 2^24, so both orders give the same sum and the same quotient.

The region is the one of tests/test_gpu_resize.py (resizes, a clipped stamp, a quick break), the Halo scene the one of
tests/test_gpu_halo_frames.py (tests/halo_frames_common.py).
"""
import gzip
import os
import numpy as np
import pytest
from scipy.special import erf
import halo_frames_common as hfc

pytestmark = pytest.mark.gpu

BLOCK = 2880


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _region(seed=3, R=110, C=96, T=24):
	"""The region of tests/test_gpu_resize.py: frames ``(R, C, T)``."""
	rng = np.random.default_rng(seed)
	row0, col0 = 200, 300
	# (row, column, tmag, trail half-length in rows): CCD coordinates
	stars = [
		(row0 + 30.3, col0 + 25.6, 11.0, 0), (row0 + 31.9, col0 + 60.2, 9.5, 0), (row0 + 70.4, col0 + 20.7, 12.5, 0),   # faint, 15x15
		(row0 + 60.2, col0 + 50.4, 6.5, 15),     # bleed trail longer than the 19x19 default stamp: one or two resizes
		(row0 + 85.7, col0 + 75.1, 6.8, 30),     # trail into the upper frame limit: "Could not resize stamp any further."
		(row0 + 12.1, col0 + 80.3, 5.5, 40),     # bright (Tmag < 6): 10 attempts, trail into the lower limit: haloswitch quick break
		(row0 + 45.5, col0 + 8.2, 10.2, 0),      # close to the left limit: default stamp clipped
		(row0 + 33.0, col0 + 27.9, 12.0, 0),     # neighbour inside the first target's stamp (skip_targets / contamination)
	]
	rr, cc = np.arange(R) + row0, np.arange(C) + col0
	img = np.zeros((R, C))
	for (r, c, tmag, trail) in stars:
		flux = 10**(-0.4 * (tmag - 20.451))
		sig = 0.6 if trail else 0.9
		pr = 0.5 * (erf((rr + 0.5 - r) / (np.sqrt(2) * sig)) - erf((rr - 0.5 - r) / (np.sqrt(2) * sig)))
		pc = 0.5 * (erf((cc + 0.5 - c) / (np.sqrt(2) * sig)) - erf((cc - 0.5 - c) / (np.sqrt(2) * sig)))
		img += flux * np.outer(pr, pc)
		if trail:
			ri, ci = int(round(r)) - row0, int(round(c)) - col0
			lo, hi = max(ri - trail, 0), min(ri + trail + 1, R)
			img[lo:hi, ci:ci + 2] += 0.02 * flux
	bkg = 100.0
	cube = img[:, :, None] * (1 + 1e-3 * rng.normal(size=T))[None, None, :]
	noise = np.sqrt(np.abs(cube) + bkg + 100.0)
	images = (cube + 30.0 + rng.normal(size=cube.shape) * noise).astype('float32')
	images[rng.random(images.shape) < 5e-4] = np.nan
	frames = {'images': images, 'images_err': noise.astype('float32'), 'backgrounds': np.full(images.shape, bkg, dtype='float32')}
	time = 1500.0 + np.arange(T) * 1800.0 / 86400.0
	quality = np.zeros(T, dtype='int32')
	quality[5] = 32
	cat = {'starid': np.arange(len(stars), dtype='int64') + 101, 'tmag': np.array([s[2] for s in stars], dtype='float32'),
		'row': np.array([s[0] for s in stars], dtype='float32'), 'column': np.array([s[1] for s in stars], dtype='float32')}
	targets = {'starid': cat['starid'].copy(), 'tmag': np.array([s[2] for s in stars]), 'row': np.array([s[0] for s in stars]),
		'column': np.array([s[1] for s in stars])}
	return frames, row0, col0, time, quality, cat, targets


# ---- a file in its parts -------------------------------------------------------------------------------------------------------
def _hdus(path):
	"""The decompressed file as a list of ``(header dict, cards, data unit with its padding)``."""
	from photometry_amd import fitsio
	with gzip.open(path, 'rb') as fh:
		blob = fh.read()
	out, pos = [], 0

	def next_block():
		nonlocal pos
		pos += BLOCK
		return blob[pos - BLOCK:pos]
	while pos < len(blob):
		header, cards = fitsio.read_header_blocks(next_block)
		_shape, nbytes = fitsio.data_unit_bytes(header)
		padded = -(-nbytes // BLOCK) * BLOCK
		out.append((header, cards, blob[pos:pos + padded]))
		pos += padded
	assert pos == len(blob)
	return out


def _without(cards, keys):
	return [c for c in cards if c[:8].strip() not in keys]


def _image(hdu):
	header, _cards, data = hdu
	shape = (header['NAXIS2'], header['NAXIS1'])
	return np.frombuffer(data, dtype='>f8', count=shape[0] * shape[1]).reshape(shape).astype('float64')


def _table(hdu):
	"""The columns of a binary-table HDU as native arrays."""
	from photometry_amd import fitsio
	header, _cards, data = hdu
	dt = np.dtype([fitsio._dtype_entry(header[f'TTYPE{i}'], header[f'TFORM{i}'], fitsio._parse_tdim(header[f'TDIM{i}']) if f'TDIM{i}' in header else None)
		for i in range(1, header['TFIELDS'] + 1)])
	rec = np.frombuffer(data, dtype=dt, count=header['NAXIS2'])
	return {name: rec[name].astype(rec[name].dtype.newbyteorder('=')) for name in dt.names}


def _hold_files(batch_path, plugin_path, sumimage, label):
	"""The two files by the rule of the module's docstring; ``sumimage``: what the batch's ``SUMIMAGE`` must equal bit for bit.  Every
	difference is gathered and printed with its figures; the caller asserts.  Returns a list of ``(HDU, column or None, text)``."""
	a, b = _hdus(batch_path), _hdus(plugin_path)
	assert [h[0].get('EXTNAME') for h in a] == [h[0].get('EXTNAME') for h in b], label
	problems = []
	for x, y in zip(a, b):
		name = x[0]['EXTNAME']
		skip = ('DATE', 'CHECKSUM') if name == 'PRIMARY' and x[0]['DATE'] != y[0]['DATE'] else ()
		if x[2] != y[2]:
			if x[0].get('XTENSION') == 'BINTABLE':
				ta, tb = _table(x), _table(y)
				for col in ta:
					va, vb = np.atleast_1d(ta[col]), np.atleast_1d(tb[col])
					same = (va == vb) | ((va != va) & (vb != vb)) if va.shape == vb.shape else np.zeros(1, dtype=bool)
					if not same.all():
						with np.errstate(invalid='ignore', divide='ignore'):
							rel = float(np.nanmax(np.abs(va - vb) / np.abs(vb))) if va.shape == vb.shape else float('nan')
						problems.append((name, col, f'{int((~same).sum())} of {same.size} values differ, largest relative difference {rel:.3e} = {rel / 2.0**-53:.1f} x 2^-53'))
			else:
				problems.append((name, None, f'data units differ in {int((_image(x) != _image(y)).sum()) if name == "SUMIMAGE" else -1} values'))
		cards = [c[:8].strip() for c, d in zip(_without(x[1], skip), _without(y[1], skip)) if c != d]
		if cards or len(_without(x[1], skip)) != len(_without(y[1], skip)):
			problems.append((name, None, 'cards differ: ' + ' '.join(cards)))
	mine = _image(a[[h[0]['EXTNAME'] for h in a].index('SUMIMAGE')])
	if not np.array_equal(mine.view('uint64'), np.asarray(sumimage, dtype='float64').view('uint64')):
		problems.append(('SUMIMAGE', None, 'not the crop of the region sum image'))
	for hdu, col, text in problems:
		print(f'{label}: {hdu}{"." + col if col else ""}: {text}')
	return problems


def _quality_of(path):
	from photometry_amd import fitsio
	return fitsio.read(path)[1][1]


# ---- the aperture region -----------------------------------------------------------------------------------------------------
def test_batch_files_equal_the_plugin_files(ctx, tmp_path):
	from photometry_amd import pipeline, tessphot_frames, STATUS
	from photometry_amd.lcfile import FileInfo, CORRECTOR_BACKGROUND_SHENANIGANS
	from photometry_amd.plugins import AperturePhotometry
	from photometry_amd.tessphot import run_plugin
	from photometry_amd.source import MemoryStampSource
	frames, row0, col0, time, quality, cat, targets = _region()
	R, C, T = frames['images'].shape
	n = len(targets['starid'])
	rng = np.random.default_rng(8)
	fr = {k: np.ascontiguousarray(np.moveaxis(v, 2, 0)) for k, v in frames.items()}
	# the final stamps (the pixel flags take no part in the photometry): where the flags of the case go
	plain = tessphot_frames(ctx, pipeline.FrameStack(ctx, fr, row0, col0), targets, cat, time, quality)
	st0, st2 = (tuple(int(v) for v in plain.stamp[i]) for i in (0, 2))
	assert plain.filepaths is None
	flags = rng.integers(0, 4, (T, R, C)).astype('uint8')                       # bits 1 and 2 scattered everywhere
	flags[3, st0[0] - row0, st0[2] - col0] |= 4                                   # bit 4 inside target 0's stamp: its first pixel ...
	flags[7, st0[1] - 1 - row0, st0[3] - 1 - col0] |= 4                           # ... and its last
	flags[4, st2[1] - row0, st2[2] - col0 + 3] |= 4                               # bit 4 one pixel outside target 2's final stamp
	used = rng.random((R, C)) < 0.7
	timecorr = 1e-3 * rng.normal(size=T)
	stack = pipeline.FrameStack(ctx, dict(fr, pixel_flags=flags, backgrounds_pixels_used=used), row0, col0)
	assert stack.pixel_flags is not None and stack.backgrounds_pixels_used.dtype == bool and stack.names == ('images', 'images_err', 'backgrounds')
	src = MemoryStampSource(dict(frames, pixel_flags=np.moveaxis(flags, 0, 2)), row0, col0, time, timecorr, np.arange(T), quality, cat, targets=targets,
		backgrounds_pixels_used=used, sector=14, camera=2, ccd=3)
	a, b = tmp_path / 'batch', tmp_path / 'plugin'
	batch = tessphot_frames(ctx, stack, targets, cat, time, quality, timecorr=timecorr, cadenceno=np.arange(T), output_folder=str(a), fileinfo=FileInfo.from_source(src), version=6)
	np.testing.assert_array_equal(batch.status, plain.status)
	np.testing.assert_array_equal(batch.stamp, plain.stamp)
	with_file = []
	for i in range(n):
		p = run_plugin(AperturePhotometry, int(targets['starid'][i]), src, str(b), ctx=ctx)
		wrote = 'filepath_lightcurve' in p._details
		assert wrote == (batch.filepaths[i] is not None) == (batch.status[i] in (STATUS.OK.value, STATUS.WARNING.value)), (i, p.status, batch.status[i])
		assert ('filepath_lightcurve' in batch[i]._details) == wrote
		if wrote:
			assert batch[i]._details['filepath_lightcurve'] == p._details['filepath_lightcurve'] == os.path.basename(batch.filepaths[i])
			assert os.path.dirname(batch.filepaths[i]) == str(a)
			with_file.append(i)
	assert len(with_file) >= 5 and 0 in with_file and 2 in with_file
	assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == len(with_file)
	for i in with_file:
		name = os.path.basename(batch.filepaths[i])
		problems = _hold_files(str(a / name), str(b / name), batch.frames[i]['sumimage'], f'target {i}')
		assert not problems, (i, problems)
		tab = _quality_of(str(a / name))
		assert len(tab['QUALITY']) == T
		want = [3, 7] if i == 0 else [] if i == 2 else None
		if want is not None:
			assert np.flatnonzero(tab['QUALITY']).tolist() == want and set(tab['QUALITY'][want].tolist()) <= {CORRECTOR_BACKGROUND_SHENANIGANS}, (i, tab['QUALITY'])
		assert tab['PIXEL_QUALITY'][5] == 32
		np.testing.assert_array_equal(tab['TIMECORR'], timecorr.astype('float32'))


def test_no_flags_and_movement_kernels(ctx, tmp_path):
	"""A stack without pixel flags: ``QUALITY`` all zero; ``movement=``: ``POS_CORR1/2`` are ``results.pos_corr``."""
	from photometry_amd import pipeline, tessphot_frames, STATUS
	from photometry_amd.lcfile import FileInfo
	from photometry_amd.motion import MovementKernel
	frames, row0, col0, time, quality, cat, targets = _region()
	T = len(time)
	rng = np.random.default_rng(9)
	timecorr = 1e-3 * rng.normal(size=T)
	mk = MovementKernel('translation')
	mk.load_series(time - timecorr, 0.05 * rng.normal(size=(T, 2)))
	stack = pipeline.FrameStack(ctx, {k: np.ascontiguousarray(np.moveaxis(v, 2, 0)) for k, v in frames.items()}, row0, col0)
	assert stack.pixel_flags is None and stack.backgrounds_pixels_used is None
	res = tessphot_frames(ctx, stack, targets, cat, time, quality, timecorr=timecorr, movement=mk, output_folder=str(tmp_path), fileinfo=FileInfo(14, 2, 3), version=6)
	assert res.pos_corr is not None and np.any(res.pos_corr != 0)
	n_files = 0
	for i, path in enumerate(res.filepaths):
		assert (path is not None) == (res.status[i] in (STATUS.OK.value, STATUS.WARNING.value))
		if path is None:
			continue
		tab = _quality_of(path)
		assert not tab['QUALITY'].any() and len(tab['QUALITY']) == T
		np.testing.assert_array_equal(tab['POS_CORR1'], res.pos_corr[i][:, 0])
		np.testing.assert_array_equal(tab['POS_CORR2'], res.pos_corr[i][:, 1])
		np.testing.assert_array_equal(tab['FLUX_RAW'].view('uint64'), res[i].lightcurve['flux'].view('uint64'))
		n_files += 1
	assert n_files >= 5
	# the pipelined entry writes each batch as it is collected: the same files
	from photometry_amd import tessphot_frames_pipelined
	halves = [{k: np.asarray(v)[:3] for k, v in targets.items()}, {k: np.asarray(v)[3:] for k, v in targets.items()}]
	parts = list(tessphot_frames_pipelined(ctx, stack, halves, cat, time, quality, timecorr=timecorr, movement=mk, output_folder=str(tmp_path / 'pipelined'),
		fileinfo=FileInfo(14, 2, 3), version=6))
	again = parts[0].filepaths + parts[1].filepaths
	assert [p is None for p in again] == [p is None for p in res.filepaths]
	for i, (one, two) in enumerate(zip(res.filepaths, again)):
		if one is not None:
			assert os.path.basename(one) == os.path.basename(two) and os.path.dirname(two) == str(tmp_path / 'pipelined')
			assert not _hold_files(two, one, res.frames[i]['sumimage'], f'pipelined target {i}')


# ---- the Halo scene ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def halo_files(ctx, tmp_path_factory):
	"""The Halo scene through ``tessphot_frames`` with files and through ``tessphot(None, ...)`` per target, under ``[halo] enabled =
	true``, once: every difference between the two files of every target."""
	from photometry_amd import pipeline, tessphot, tessphot_frames, STATUS
	from photometry_amd.lcfile import FileInfo
	from photometry_amd.source import MemoryStampSource
	tmp_path = tmp_path_factory.mktemp('halo_files')
	ini = tmp_path / 'settings.ini'
	ini.write_text('[halo]\nenabled = true\n')
	before = os.environ.get('TESSPHOT_SETTINGS')
	os.environ['TESSPHOT_SETTINGS'] = str(ini)
	try:
		frames, row0, col0, time, quality, cat, targets = hfc.region()
		T, n = len(time), len(targets['starid'])
		stack = pipeline.FrameStack(ctx, {k: np.ascontiguousarray(np.moveaxis(v, 2, 0)) for k, v in frames.items()}, row0, col0)
		src = MemoryStampSource(frames, row0, col0, time, np.zeros(T), np.arange(T), quality, cat, sector=2, targets=targets)
		a = tmp_path / 'batch'
		on = tessphot_frames(ctx, stack, targets, cat, time, quality, sector=2, timecorr=np.zeros(T), cadenceno=np.arange(T), output_folder=str(a),
			fileinfo=FileInfo.from_source(src), version=6)
		assert sorted(int(targets['starid'][i]) for i in on.halo_rows) == sorted(hfc.BRIGHT_SWITCHING)
		region_sum = stack.sumimage_for(quality).to_host()
		out = {'halo': 0, 'aperture': 0, 'differing': []}
		for i in range(n):
			sid = int(targets['starid'][i])
			folder = tmp_path / f'out{sid}'
			pho = tessphot(None, sid, src, str(folder), ctx=ctx)
			wrote = 'filepath_lightcurve' in pho._details
			assert wrote == (on.filepaths[i] is not None) == (on.status[i] in (STATUS.OK.value, STATUS.WARNING.value)), (sid, pho.status, on.status[i])
			if not wrote:
				continue
			name = os.path.basename(on.filepaths[i])
			assert pho._details['filepath_lightcurve'] == name == on[i]._details['filepath_lightcurve']
			stamp = tuple(int(v) for v in on.stamp[i])
			if i in on.halo_rows:
				assert pho.method == 'halo'
				sumimage = region_sum[stamp[0] - row0:stamp[1] - row0, stamp[2] - col0:stamp[3] - col0]
			else:
				sumimage = on.frames[i]['sumimage']
			out[pho.method] += 1
			out['differing'] += [(sid, pho.method) + p for p in _hold_files(str(a / name), str(folder / name), sumimage, f'starid {sid} ({pho.method})')]
			if i in on.halo_rows:
				parts = _hdus(str(a / name))
				assert [h[0]['EXTNAME'] for h in parts] == ['PRIMARY', 'LIGHTCURVE', 'SUMIMAGE', 'APERTURE', 'WEIGHTMAP']
				assert parts[0][0]['PHOTMET'] == 'halo' and parts[0][0]['NEXTEND'] == 4 and 'HALO_VER' in parts[0][0]
				assert not _quality_of(str(a / name))['FLUX_BKG'].any()
		return out
	finally:
		if before is None:
			del os.environ['TESSPHOT_SETTINGS']
		else:
			os.environ['TESSPHOT_SETTINGS'] = before


def test_switched_targets_get_the_halo_file(halo_files):
	"""Every file of the Halo scene equals ``tessphot(None, ...)``'s byte for byte: the aperture targets' files, and of the switched
	targets the primary header with ``PHOTMET`` and the ``HALO_*`` cards, the whole table -- ``FLUX_RAW_ERR`` too: the batched Halo path
	adds ``wm^2 err^2`` up in the order of the per-target path's ``nansum`` --, ``SUMIMAGE``, ``APERTURE`` and ``WEIGHTMAP``."""
	assert halo_files['halo'] == len(hfc.BRIGHT_SWITCHING) and halo_files['aperture'] >= 3
	assert not halo_files['differing'], halo_files['differing']
