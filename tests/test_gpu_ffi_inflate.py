# -*- coding: utf-8 -*-
"""
``ffi.load_ffis(inflate='device')``: ``.fits.gz`` files inflated on the device in batches (``tp_inflate``) and unpacked in place, held
bit for bit to ``ffi.load_ffis()`` on the same files -- today's path, the host's ``gzip``.  Files from tests/ffi_common.py: small ones
that are not from TESS (the image in the primary HDU: the header behind it comes from the inflated bytes) and small ones laid out as
TESS files are (primary without data).  Broken files raise ``ffi.InflateError`` naming the file and leave nothing allocated.
"""
import gzip
import logging
import os
import numpy as np
import pytest
import ffi_common as fc
from alloc_common import count_allocations
from photometry_amd import ffi

pytestmark = pytest.mark.gpu

STEP = 1800.0 / 86400.0
T0 = 1325.317007851970
SHAPE = (37, 53)
NAMES = ['tess2018206%06d-s0001-1-1-0120-s_ffic.fits' % (45240 + 3000 * k) for k in range(6)]


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _blob(k, rng, shape=SHAPE, datasum=True):
	"""File k: the image in the primary HDU, uncertainty and WCS in the first extension; a long run of COMMENT cards in file 3 puts
	the uncertainty header's END into its seventh block."""
	rr, cc = np.mgrid[0:shape[0], 0:shape[1]]
	img = (100.0 + 0.3 * rr + 0.1 * cc + rng.normal(size=shape)).astype('float32')
	unc = np.sqrt(img).astype('float32')
	img[3, 5], unc[4, 6] = np.nan, np.inf
	cards = [fc.card('TSTART', T0 + k * STEP), fc.card('TSTOP', T0 + (k + 1) * STEP), fc.card('CAMERA', 1), fc.card('CCD', 2), fc.card('NUM_FRM', 900),
		fc.card('BARYCORR', 0.001 * (k + 1)), fc.card('DQUALITY', 4 if k == 3 else 0)]
	ext = fc.tan_cards(crval=(120.0 + 1e-4 * k, -35.0)) + (['COMMENT filler'.ljust(80)] * 220 if k == 3 else [])
	return fc.plain_file(img, unc, primary_cards=cards, ext_cards=ext, datasum=datasum)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
	root = tmp_path_factory.mktemp('ffigz')
	rng = np.random.default_rng(31)
	blobs = [_blob(k, rng, datasum=k != 2) for k in range(5)]
	return {'root': root, 'blobs': blobs, 'gz': [fc.write(root / (NAMES[k] + '.gz'), b) for k, b in enumerate(blobs)],
		'plain': [fc.write(root / NAMES[k], b) for k, b in enumerate(blobs)]}


def _equal(a, b):
	for name in ('raw', 'raw_err'):
		x, y = getattr(a, name).to_host(), getattr(b, name).to_host()
		assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view('uint32'), y.view('uint32')), name
	for name in ('time', 'time_start', 'time_stop', 'timecorr', 'quality', 'cadenceno'):
		x, y = getattr(a, name), getattr(b, name)
		assert x.dtype == y.dtype and np.array_equal(x, y), name
	assert a.wcs_headers == b.wcs_headers and a.attributes == b.attributes and a.backapp == b.backapp and a.files == b.files
	assert (a.row_offset, a.col_offset, a.is_tess) == (b.row_offset, b.col_offset, b.is_tess)
	assert set(a.headers) == set(b.headers) and all(np.array_equal(a.headers[k], b.headers[k]) for k in a.headers)


def test_five_gz_files_in_batches_of_two(ctx, files, monkeypatch):
	launches = []
	inflate_entry = ctx.lib.tp_inflate
	monkeypatch.setattr(ctx.lib, 'tp_inflate', lambda *args: (launches.append(int(args[3])), inflate_entry(*args))[1])
	want = ffi.load_ffis(ctx, files['gz'])
	assert launches == []                                                            # the default is the host's inflate
	got = ffi.load_ffis(ctx, files['gz'], inflate='device', batch_files=2)
	assert launches == [4, 4, 2]                                                     # (a file is a stream and the bytes up to the next one)
	_equal(got, want)
	assert got.stats['inflate_files'] == 5 and got.stats['host_files'] == 0 and got.stats['inflate_wait_s'] > 0
	assert got.stats['bytes'] == sum(os.path.getsize(f) for f in files['gz'])         # the compressed bytes are what is read
	assert 'A_ORDER' not in got.wcs_headers[3] and all('CTYPE1  =' in h for h in got.wcs_headers)
	# the default batch: one launch
	del launches[:]
	_equal(ffi.load_ffis(ctx, files['gz'], inflate='device'), want)
	assert launches == [10]
	for x in (got, want):
		x.free()


def test_mixed_list_and_prepare(ctx, files):
	mixed = [files['plain'][0], files['gz'][1], files['gz'][2], files['plain'][3], files['gz'][4]]
	want = ffi.load_ffis(ctx, mixed)
	got = ffi.load_ffis(ctx, mixed, inflate='device', batch_files=2)
	_equal(got, want)
	assert got.stats['inflate_files'] == 3
	a = ffi.prepare_ffis(ctx, files['gz'], cadence=1800, inflate='device')
	b = ffi.prepare_ffis(ctx, files['gz'], cadence=1800)
	for name in ('images', 'images_err', 'backgrounds', 'pixel_flags'):
		assert np.array_equal(a[name].to_host().view('uint8'), b[name].to_host().view('uint8')), name
	assert a['loaded'].stats['inflate_files'] == 5 and a['ref_frame'] == b['ref_frame']
	for x in (got, want, a['loaded'], b['loaded']):
		x.free()


def test_an_empty_primary_is_refused_by_both_paths_alike(ctx, tmp_path):
	"""Primary without data: two headers lie in front of the first data unit, and both come from the file's first KBs.  (The layout of a
	TESS file; being one takes the full 2078 x 2136 frame, whose front tests/test_ffi_inflate_host.py reads.)"""
	rng = np.random.default_rng(5)
	paths = []
	for k in range(2):
		img = rng.normal(100, 3, SHAPE).astype('float32')
		primary = fc.hdu([fc.card('SIMPLE', True), fc.card('BITPIX', 8), fc.card('NAXIS', 0), fc.card('EXTEND', True), fc.card('TSTART', T0 + k * STEP), fc.card('TSTOP', T0 + (k + 1) * STEP)], datasum=False)
		ext = [fc.hdu(fc.image_cards(fc.card('XTENSION', 'IMAGE'), -32, SHAPE) + [fc.card('PCOUNT', 0), fc.card('GCOUNT', 1)] + fc.tan_cards(), fc.be_bytes(a, -32))
			for a in (img, np.sqrt(img))]
		# (not a TESS file: the image is HDU 0, which has no data -- refused by both paths alike)
		paths.append(fc.write(tmp_path / (NAMES[k] + '.gz'), primary + ext[0] + ext[1]))
	for how in ({}, {'inflate': 'device'}):
		with pytest.raises(ValueError, match='not a float image'):
			ffi.load_ffis(ctx, paths, **how)


def test_two_members_go_the_host_way(ctx, files, caplog, monkeypatch):
	# (the front the host inflates ends with the primary header here, as it does in a file whose first member is longer than the front:
	# that a second member follows shows only once the device has inflated the first)
	monkeypatch.setattr(ffi, 'FRONT_INFLATED', fc.BLOCK)
	root = files['root']
	blob = files['blobs'][1]
	small_tail = str(root / ('two_a_' + NAMES[1] + '.gz'))
	large_tail = str(root / ('two_b_' + NAMES[1] + '.gz'))
	padded = str(root / ('pad_' + NAMES[1] + '.gz'))
	cut = len(blob) - 2000
	with open(small_tail, 'wb') as fh:                                               # the last member is smaller than the headers' span: known from the front
		fh.write(gzip.compress(blob[:cut], 1) + gzip.compress(blob[cut:], 1))
	with open(large_tail, 'wb') as fh:                                               # the last member says enough bytes: known once the first stream has ended early
		fh.write(gzip.compress(blob[:3000], 1) + gzip.compress(blob[3000:], 1))
	with open(padded, 'wb') as fh:                                                   # bytes behind the final block other than the trailer
		member = gzip.compress(blob, 1)
		fh.write(member[:-8] + b'\x00' * 5 + member[-8:])
	want = ffi.load_ffis(ctx, [files['gz'][0], files['gz'][1]])
	for odd, host_is_fine in ((small_tail, True), (large_tail, True), (padded, False)):
		with caplog.at_level(logging.INFO, logger='photometry_amd.ffi'):
			caplog.clear()
			if host_is_fine:
				got = ffi.load_ffis(ctx, [files['gz'][0], odd], inflate='device')
				assert got.stats['inflate_files'] == 1 and got.stats['host_files'] == 1
				got.files = want.files
				_equal(got, want)
				got.free()
			else:
				with pytest.raises(ffi.InflateError) as e:                           # the host's gzip does not take it either: its complaint, naming the file
					ffi.load_ffis(ctx, [files['gz'][0], odd], inflate='device')
				assert odd in str(e.value)
		assert any("goes through the host's inflate" in r.getMessage() and odd in r.getMessage() for r in caplog.records), odd
	want.free()


def _broken(files, tmp_path):
	raw = open(files['gz'][2], 'rb').read()
	flipped = bytearray(raw)
	flipped[len(raw) // 2] ^= 0x40
	crc = bytearray(raw)
	crc[-6] ^= 0x01
	return {'flipped': bytes(flipped), 'cut': raw[:len(raw) * 2 // 3], 'crc': bytes(crc)}


@pytest.mark.parametrize('what', ['flipped', 'cut', 'crc'])
def test_broken_files_raise_and_leave_nothing(ctx, files, tmp_path, monkeypatch, what):
	path = str(tmp_path / (NAMES[2] + '.gz'))
	with open(path, 'wb') as fh:
		fh.write(_broken(files, tmp_path)[what])
	live = count_allocations(ctx, monkeypatch)
	with pytest.raises(ffi.InflateError) as e:
		ffi.load_ffis(ctx, [files['gz'][0], files['gz'][1], path, files['gz'][3]], inflate='device', batch_files=3)
	assert path in str(e.value) and isinstance(e.value, ValueError) and e.value.index == 2 and e.value.status
	if what == 'crc':
		assert e.value.status == 'CRC'
	assert live == {'device': 0, 'host': 0}, live
	if what == 'crc':                                                                # unverified, the same file loads: file 2 has no DATASUM cards
		loaded = ffi.load_ffis(ctx, [path], inflate='device', verify=False)
		assert live == {'device': 2, 'host': 0}, live
		loaded.free()


def test_a_wrong_datasum_still_raises_checksum_error(ctx, files, tmp_path, monkeypatch):
	blob = bytearray(files['blobs'][1])
	h = ffi.read_ffi_header(files['plain'][1])
	blob[h.uncert.offset + 4 * 7 + 2] ^= 0x08
	path = fc.write(tmp_path / (NAMES[1] + '.gz'), bytes(blob))                      # a sound gzip file of unsound FITS
	live = count_allocations(ctx, monkeypatch)
	with pytest.raises(ffi.ChecksumError) as e:
		ffi.load_ffis(ctx, [files['gz'][0], path], inflate='device')
	assert path in str(e.value) and 'HDU 1' in str(e.value)
	assert live == {'device': 0, 'host': 0}, live


def test_another_shape_in_the_third_file_is_refused_before_any_allocation(ctx, files, tmp_path, monkeypatch):
	odd = fc.write(tmp_path / (NAMES[5] + '.gz'), _blob(5, np.random.default_rng(1), shape=(40, 53)))

	def no_allocation(*args, **kwargs):
		raise AssertionError('allocated before the shapes were checked')
	for name in ('empty', 'zeros', 'pinned', 'pinned_block'):
		monkeypatch.setattr(ctx, name, no_allocation)
	with pytest.raises(ValueError) as e:
		ffi.load_ffis(ctx, files['gz'][:2] + [odd] + files['gz'][2:], inflate='device')
	assert odd in str(e.value) and not isinstance(e.value, ffi.InflateError)
