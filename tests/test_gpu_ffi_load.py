# -*- coding: utf-8 -*-
"""
``photometry_amd.ffi`` on the device: ``load_ffis`` on three TESS-shaped files and on small files that are not from TESS (all written
by tests/ffi_common.py, not by ``photometry_amd.fitsio``), held bit for bit to numpy's crop of the same arrays, and ``prepare_ffis``
held to ``prepare.prepare_frames`` fed with the numpy-unpacked inputs.
"""
import logging
import os
import numpy as np
import pytest
import ffi_common as fc
from alloc_common import count_allocations
from photometry_amd import ffi, frameio, motion, prepare

pytestmark = pytest.mark.gpu

STEP = 1800.0 / 86400.0
T0 = 1325.317007851970
NAMES = ['tess2018206%06d-s0001-1-1-0120-s_ffic.fits' % (45240 + 3000 * k) for k in range(4)]


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _same_bits(a, b):
	a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
	return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view('uint8'), b.view('uint8'))


# ---- three TESS-shaped files --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tess_set(tmp_path_factory):
	"""Random bit patterns in every pixel of image and uncertainty; file 2 lacks BARYCORR and DQUALITY."""
	root = tmp_path_factory.mktemp('tess')
	rng = np.random.default_rng(2024)
	files, bits, blobs = [], [], []
	for k in range(3):
		img = rng.integers(0, 2**32, size=fc.TESS_SHAPE, dtype='uint64').astype('uint32')
		unc = rng.integers(0, 2**32, size=fc.TESS_SHAPE, dtype='uint64').astype('uint32')
		cards = [fc.card('TSTART', T0 + k * STEP), fc.card('TSTOP', T0 + (k + 1) * STEP), fc.card('EXPOSURE', 0.0165), fc.card('FFIINDEX', 4697 + k)]
		if k < 2:
			cards += [fc.card('BARYCORR', 0.0039 + 0.0001 * k), fc.card('DQUALITY', 32 * k)]
		primary = [fc.card('CAMERA', 1), fc.card('CCD', 4), fc.card('DATA_REL', 5), fc.card('PROCVER', 'spoc-4.0.5'), fc.card('NUM_FRM', 900), fc.card('CRMITEN', True)]
		blob = fc.tess_file(img, unc, cards, primary_cards=primary, ext_cards=fc.tan_cards(crpix=(1045.0, 1001.0)))
		files.append(fc.write(root / NAMES[k], blob))
		bits.append((img, unc))
		blobs.append(blob)
	return {'root': str(root), 'files': files, 'bits': bits, 'blobs': blobs}


@pytest.fixture(scope='module')
def tess_loaded(ctx, tess_set):
	order = [2, 0, 1]
	loaded = ffi.load_ffis(ctx, [tess_set['files'][k] for k in order])
	return order, loaded, loaded.raw.to_host(), loaded.raw_err.to_host()


def test_tess_stacks_are_the_numpy_crop_in_the_order_given(tess_set, tess_loaded):
	order, loaded, raw, raw_err = tess_loaded
	assert raw.shape == raw_err.shape == (3, 2048, 2048) and raw.dtype == raw_err.dtype == np.float32
	for j, k in enumerate(order):
		img, unc = tess_set['bits'][k]
		assert np.array_equal(raw[j].view('uint32'), img[0:2048, 44:2092]), (j, k)
		assert np.array_equal(raw_err[j].view('uint32'), unc[0:2048, 44:2092]), (j, k)
	assert (loaded.row_offset, loaded.col_offset) == (0, 44) and loaded.is_tess
	assert loaded.stats['bytes'] == 3 * (2 * 17755200 + 2880)              # image unit, the uncertainty's header block, uncertainty unit


def test_tess_vectors_headers_and_defaults(tess_set, tess_loaded):
	order, loaded, _, _ = tess_loaded
	k = np.array(order)
	assert np.array_equal(loaded.time_start, T0 + k * STEP) and np.array_equal(loaded.time_stop, T0 + (k + 1) * STEP)
	assert np.array_equal(loaded.time, 0.5 * ((T0 + k * STEP) + (T0 + (k + 1) * STEP))) and loaded.time.dtype == np.float64
	assert np.array_equal(loaded.timecorr, np.array([0.0, 0.0039, 0.0040], dtype='float32')) and loaded.timecorr.dtype == np.float32    # default 0
	assert np.array_equal(loaded.quality, [0, 0, 32]) and loaded.quality.dtype == np.int32                                                # default 0
	assert np.array_equal(loaded.cadenceno, 4697 + k) and loaded.cadenceno.dtype == np.int32
	h = loaded.headers
	assert h['is_tess'] is True and h['CAMERA'] == 1 and h['CCD'] == 4
	assert np.array_equal(h['FFIINDEX'], 4697 + k) and np.array_equal(h['TSTART'], loaded.time_start) and np.array_equal(h['TSTOP'], loaded.time_stop)
	assert set(h) == {'is_tess', 'CAMERA', 'CCD', 'FFIINDEX', 'TSTART', 'TSTOP'}
	assert loaded.attributes == {'CAMERA': 1, 'CCD': 4, 'DATA_REL': 5, 'PROCVER': 'spoc-4.0.5', 'NUM_FRM': 900, 'NREADOUT': None, 'CRMITEN': True, 'CRBLKSZ': None,
		'CRSPOC': None}
	assert loaded.backapp is False
	assert len(loaded.wcs_headers) == 3 and all(len(s) % 80 == 0 and 'CTYPE1  =' in s and 'CTYPE1P' not in s and 'TSTART' not in s for s in loaded.wcs_headers)
	# name order from the directory search, whatever order the files were loaded in
	assert ffi.find_ffi_files(tess_set['root']) == tess_set['files']
	assert ffi.find_ffi_files(tess_set['root'], sector=1, camera=1, ccd=1) == tess_set['files'] and ffi.find_ffi_files(tess_set['root'], sector=2) == []


@pytest.mark.parametrize('hdu,row,col', [(1, 5, 10), (2, 2060, 100)])
def test_a_flipped_byte_outside_the_science_window(ctx, tess_set, tmp_path, monkeypatch, hdu, row, col):
	blob = bytearray(tess_set['blobs'][0])
	h = ffi.read_ffi_header(tess_set['files'][0])
	unit = h.image if hdu == 1 else h.uncert
	blob[unit.offset + 4 * (row * 2136 + col) + 1] ^= 0x10
	path = fc.write(tmp_path / NAMES[0], bytes(blob))
	live = count_allocations(ctx, monkeypatch)                             # every allocation and release on ctx, device and page-locked
	with pytest.raises(ffi.ChecksumError) as e:
		ffi.load_ffis(ctx, [path])
	assert path in str(e.value) and f'HDU {hdu}' in str(e.value) and f'HDU {3 - hdu}' not in str(e.value)
	assert live == {'device': 0, 'host': 0}, live
	loaded = ffi.load_ffis(ctx, [path], verify=False)                      # the same file loads unverified: the window is untouched
	assert live == {'device': 2, 'host': 0}, live                          # the counter counts: the two stacks
	img, unc = tess_set['bits'][0]
	assert np.array_equal(loaded.raw.to_host()[0].view('uint32'), img[0:2048, 44:2092])
	assert np.array_equal(loaded.raw_err.to_host()[0].view('uint32'), unc[0:2048, 44:2092])
	loaded.free()
	assert live == {'device': 0, 'host': 0}, live


def test_tess_files_without_ffiindex(ctx, tess_set, tmp_path):
	"""Short exposures get no extrapolated FFIINDEX: TESS data without a cadence number is refused (prepare.py:402-403)."""
	blob = tess_set['blobs'][0].replace(fc.card('FFIINDEX', 4697).encode(), fc.card('FFIXNDEX', 4697).encode()).replace(
		fc.card('EXPOSURE', 0.0165).encode(), fc.card('EXPOSURE', 0.0010).encode())
	path = fc.write(tmp_path / NAMES[0], blob)
	with pytest.raises(RuntimeError, match='CADENCENO'):
		ffi.load_ffis(ctx, [path], verify=False)


# ---- small files that are not from TESS ---------------------------------------------------------------------------------------------
def _small_set(root, shape, rng, gz=False, bad_wcs=1, times=None, num_frm=(900, 900, 900, 901)):
	"""Four files: the image in the primary HDU, the uncertainty and the WCS in the first extension.  File 2 has neither BARYCORR nor
	DQUALITY nor DATASUM cards; file ``bad_wcs`` a WCS that fails the footprint check; file 3 another NUM_FRM and quality 4."""
	os.makedirs(root, exist_ok=True)
	rr, cc = np.mgrid[0:shape[0], 0:shape[1]]
	files, arrays = [], []
	for k in range(4):
		img = (100.0 + 0.3 * rr + 0.1 * cc + 50.0 * np.exp(-0.5 * ((rr - 9 - 0.1 * k)**2 + (cc - 11)**2) / 2.0) + rng.normal(size=shape)).astype('float32')
		unc = np.sqrt(img).astype('float32')
		img[3, 5], unc[4, 6] = np.nan, np.inf
		t = (T0 + k * STEP) if times is None else times[k]
		cards = [fc.card('TSTART', t), fc.card('TSTOP', t + STEP), fc.card('CAMERA', 1), fc.card('CCD', 2), fc.card('NUM_FRM', num_frm[k])]
		if k != 2:
			cards += [fc.card('BARYCORR', 0.001 * (k + 1)), fc.card('DQUALITY', 4 if k == 3 else 0)]
		wcs = fc.sip_bad_cards() if k == bad_wcs else fc.tan_cards(crval=(120.0 + 1e-4 * k, -35.0))
		name = NAMES[k] + ('.gz' if gz else '')
		files.append(fc.write(os.path.join(root, name), fc.plain_file(img, unc, primary_cards=cards, ext_cards=wcs, datasum=k != 2)))
		arrays.append((img, unc))
	return files, np.stack([a for a, _ in arrays]), np.stack([b for _, b in arrays])


@pytest.fixture(scope='module')
def small_set(tmp_path_factory):
	root = tmp_path_factory.mktemp('small')
	out = {}
	for shape in ((20, 24), (72, 80)):
		files, raw, err = _small_set(str(root / ('%dx%d' % shape)), shape, np.random.default_rng(shape[0]))
		gz, _, _ = _small_set(str(root / ('gz%dx%d' % shape)), shape, np.random.default_rng(shape[0]), gz=True)
		out[shape] = {'files': files, 'gz': gz, 'raw': raw, 'err': err}
	return out


def test_small_files_and_their_gz_copies(ctx, small_set, caplog):
	s = small_set[(20, 24)]
	with caplog.at_level(logging.ERROR, logger='photometry_amd.ffi'):
		loaded = ffi.load_ffis(ctx, s['files'])
	assert _same_bits(loaded.raw.to_host(), s['raw']) and _same_bits(loaded.raw_err.to_host(), s['err'])
	assert (loaded.row_offset, loaded.col_offset) == (0, 0) and not loaded.is_tess and loaded.headers['is_tess'] is False
	assert np.array_equal(loaded.cadenceno, [1, 2, 3, 4]) and loaded.headers['FFIINDEX'] is None           # k + 1 without the card
	assert np.array_equal(loaded.timecorr, np.array([0.001, 0.002, 0.0, 0.004], dtype='float32')) and np.array_equal(loaded.quality, [0, 0, 0, 4])
	assert np.allclose(loaded.time, T0 + (np.arange(4) + 0.5) * STEP, rtol=0, atol=1e-9)
	assert np.array_equal(loaded.time, 0.5 * (loaded.time_start + loaded.time_stop))
	# a card that is not the same in every file is logged as an error, as in the reference
	msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
	assert len(msgs) == 1 and 'NUM_FRM is not constant' in msgs[0] and '0003' in msgs[0]
	# file 1 carries the divergent header, every other a TAN one; only WCS keywords are kept
	assert all('CTYPE1  =' in h and 'TSTART' not in h and 'CTYPE1P' not in h for h in loaded.wcs_headers) and 'A_ORDER' in loaded.wcs_headers[1]
	gz = ffi.load_ffis(ctx, s['gz'])
	assert _same_bits(gz.raw.to_host(), s['raw']) and _same_bits(gz.raw_err.to_host(), s['err'])
	assert np.array_equal(gz.time, loaded.time) and gz.wcs_headers == loaded.wcs_headers
	for x in (loaded, gz):
		x.free()


def test_a_file_of_another_shape_is_refused_before_any_allocation(ctx, small_set, tess_set, monkeypatch):
	def no_allocation(*args, **kwargs):
		raise AssertionError('allocated before the shapes were checked')
	for name in ('empty', 'zeros', 'pinned'):
		monkeypatch.setattr(ctx, name, no_allocation)
	odd = small_set[(72, 80)]['files'][1]
	with pytest.raises(ValueError) as e:
		ffi.load_ffis(ctx, small_set[(20, 24)]['files'][:2] + [odd])
	assert odd in str(e.value)
	with pytest.raises(ValueError) as e:
		ffi.load_ffis(ctx, [tess_set['files'][0], odd])
	assert odd in str(e.value)


@pytest.mark.parametrize('shape', [(20, 24), (72, 80)])
def test_prepare_ffis_equals_prepare_frames_on_numpy_inputs(ctx, small_set, tmp_path, shape):
	s = small_set[shape]
	quality = np.array([0, 0, 0, 4], dtype='int32')
	tstart = T0 + np.arange(4) * STEP
	time = 0.5 * (tstart + (tstart + STEP))
	path = str(tmp_path / 'ccd.tpstack')
	# frame 1 is nearest the reference time but has a WCS that fails the footprint check; frame 3 has a bad quality
	out = ffi.prepare_ffis(ctx, s['files'], reference_time=time[1] + 0.1 * STEP, write=path)
	assert out['cadence'] == 1800 and out['ref_frame'] == 2 and out['path'] == path
	assert [bool(h.strip()) for h in out['wcs_headers']] == [True, False, True, True] and out['wcs_headers'][1] == ''
	headers = {'is_tess': False, 'CAMERA': 1, 'CCD': 2, 'FFIINDEX': None, 'TSTART': tstart, 'TSTOP': tstart + STEP}
	want = prepare.prepare_frames(ctx, ctx.array(s['raw']), ctx.array(s['err']), quality, cadence=1800, headers=headers)
	names = ('backgrounds', 'images', 'images_err', 'sumimage', 'pixel_flags', 'backgrounds_pixels_used')
	assert set(names) <= set(out) and set(names) == set(want)
	host = {}
	for name in names:
		host[name] = out[name].to_host()
		assert _same_bits(host[name], want[name].to_host()), name
	if shape == (72, 80):
		assert np.isfinite(host['backgrounds']).any() and np.isfinite(host['sumimage']).any()      # (a 20 x 24 frame fills too little of its one 64 x 64 mesh cell)
	# the written stack comes back through load_stack, with everything the later stages read
	groups, meta = frameio.load_stack(ctx, path, groups=('images', 'images_err', 'backgrounds', 'pixel_flags'))
	for name, d in groups.items():
		assert _same_bits(d.to_host(), host[name]), name
	assert meta['shape'] == [4, shape[0], shape[1]] and (meta['row_offset'], meta['col_offset']) == (0, 0)
	assert np.array_equal(meta['time'], time) and meta['cadenceno'] == [1, 2, 3, 4] and meta['quality'] == [0, 0, 0, 4]
	a = meta['attrs']
	assert a['TIME_OFFSET_CORRECTED'] is False and a['SECTOR'] == 1 and a['CADENCE'] == 1800 and a['CAMERA'] == 1 and a['CCD'] == 2 and a['NUM_FRM'] == 900
	assert a['time_start'] == list(tstart) and a['time_stop'] == list(tstart + STEP) and np.allclose(a['timecorr'], [0.001, 0.002, 0.0, 0.004], rtol=1e-6, atol=0)
	assert a['wcs_headers'] == out['wcs_headers'] and a['wcs_ref'] == out['wcs_headers'][2] and 'movement_kernel' not in a
	mk = motion.movement_from_header(meta)
	assert mk.warpmode == 'wcs' and np.array_equal(mk.series_times, time[[0, 2, 3]])
	jitter = mk.jitter(time[[0, 2]], 5.0, 7.0)
	assert jitter.shape == (2, 2) and np.all(np.isfinite(jitter)) and np.all(np.abs(jitter[1]) < 1e-9) and abs(jitter[0, 0]) > 1e-3


def test_prepare_ffis_refusals(ctx, small_set, tmp_path):
	s = small_set[(20, 24)]
	with pytest.raises(ValueError, match='not sorted'):
		ffi.prepare_ffis(ctx, s['files'][::-1])
	with pytest.raises(ValueError, match='not sorted'):
		ffi.prepare_ffis(ctx, [s['files'][0], s['files'][0], s['files'][2]])
	loaded = ffi.load_ffis(ctx, s['files'])
	with pytest.raises(ValueError, match='cadence of 200'):
		ffi.prepare_ffis(ctx, loaded, cadence=200)
	with pytest.raises(ValueError, match='cadence of 200'):
		ffi.prepare_ffis(ctx, loaded, sector=56)
	# the only frames with a good WCS and quality 0 are 0 and 2: a reference time at frame 3 still chooses frame 2
	out = ffi.prepare_ffis(ctx, loaded, reference_time=loaded.time[3], cadence=600)
	assert out['ref_frame'] == 2 and out['cadence'] == 600 and out['loaded'] is loaded and out['path'] is None
	loaded.quality[[0, 2]] = 8
	with pytest.raises(RuntimeError, match='refindx'):
		ffi.prepare_ffis(ctx, loaded)
	loaded.free()
