# -*- coding: utf-8 -*-
"""
CPU checks of the FFI input path: the header side of ``photometry_amd.ffi`` (``read_ffi_header``, ``find_ffi_files``, the FFIINDEX
extrapolation) on files written by tests/ffi_common.py, and the device-free rules of the unpacker (photometry_amd/csrc/fits_rules.h)
compiled for the host with AddressSanitizer and UBSan into tests/hostsim/fits_rules_host.cpp and held to Python and numpy.
"""
import os
import subprocess
import numpy as np
import pytest
import conftest
import ffi_common as fc
from photometry_amd import ffi, fitsio

CSRC = os.path.join(conftest.ROOT, 'photometry_amd', 'csrc')
SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'fits_rules_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'fits_rules_host')

TIME_CARDS = [fc.card('TSTART', 1325.317007851970), fc.card('TSTOP', 1325.337841177751), fc.card('BARYCORR', 3.9072474e-03), fc.card('EXPOSURE', 0.0165),
	fc.card('DQUALITY', 0)]


def _tess_headers_only(tmp_path, name='t.fits', primary=(), ext=(), telescop=True):
	"""A TESS-shaped file cut short behind the header of its uncertainty extension: a sparse file, its data units never written."""
	prim = [fc.card('SIMPLE', True), fc.card('BITPIX', 8), fc.card('NAXIS', 0), fc.card('EXTEND', True)]
	if telescop:
		prim.append(fc.card('TELESCOP', 'TESS'))
	h0 = fc.header_bytes(prim + list(primary))
	h1 = fc.header_bytes(fc.image_cards(fc.card('XTENSION', 'IMAGE'), -32, fc.TESS_SHAPE) + [fc.card('PCOUNT', 0), fc.card('GCOUNT', 1)] + list(ext) +
		[fc.card('DATASUM', '123456')])
	h2 = fc.header_bytes(fc.image_cards(fc.card('XTENSION', 'IMAGE'), -32, fc.TESS_SHAPE) + [fc.card('PCOUNT', 0), fc.card('GCOUNT', 1)])
	unit = -(-fc.TESS_SHAPE[0] * fc.TESS_SHAPE[1] * 4 // 2880) * 2880
	path = tmp_path / name
	with open(path, 'wb') as fh:
		fh.write(h0 + h1)
		fh.seek(len(h0) + len(h1) + unit)
		fh.write(h2)
	return str(path), len(h0), len(h1), len(h2), unit


# ---- headers ---------------------------------------------------------------------------------------------------------------------
def test_headers_and_offsets_of_a_file_without_its_data_units(tmp_path):
	path, n0, n1, n2, unit = _tess_headers_only(tmp_path, primary=[fc.card('CAMERA', 2), fc.card('CCD', 3), fc.card('ORIGIN', 'primary')],
		ext=TIME_CARDS + [fc.card('FFIINDEX', 5000), fc.card('ORIGIN', 'ext'), fc.card('CTYPE1', 'RA---TAN')])
	assert os.path.getsize(path) == n0 + n1 + unit + n2               # the uncertainty unit is not there at all
	h = ffi.read_ffi_header(path)
	assert h.is_tess
	assert h.image == ffi.DataUnit(1, n0 + n1, -32, fc.TESS_SHAPE, unit, 123456)
	assert h.uncert == ffi.DataUnit(2, n0 + n1 + unit + n2, -32, fc.TESS_SHAPE, unit, None)
	assert unit == 17755200 and unit % 2880 == 0
	# merged header: the primary's cards, the first extension's on top (io.py:51-52)
	assert h.header['CAMERA'] == 2 and h.header['CCD'] == 3 and h.header['TELESCOP'] == 'TESS'
	assert h.header['ORIGIN'] == 'ext' and h.header['XTENSION'] == 'IMAGE' and h.header['NAXIS1'] == 2136
	assert h.header['FFIINDEX'] == 5000 and h.header['TSTART'] == 1325.317007851970
	assert len(h.wcs_cards) % 80 == 0 and 'CTYPE1' in h.wcs_cards and 'CAMERA' not in h.wcs_cards
	assert ffi.wcs_header_string(h.wcs_cards) == (fc.card('NAXIS1', 2136) + fc.card('NAXIS2', 2078) + fc.card('CTYPE1', 'RA---TAN'))


def test_a_file_of_the_tess_shape_without_telescop_is_not_tess(tmp_path):
	path, n0, n1, n2, unit = _tess_headers_only(tmp_path, primary=[fc.card('ORIGIN', 'primary')], ext=TIME_CARDS + [fc.card('ORIGIN', 'ext')], telescop=False)
	h = ffi.read_ffi_header(path)
	assert not h.is_tess
	# image and uncertainty are HDU 0 and HDU 1 then (io.py:80-82), the header is the primary's alone
	assert (h.image.hdu, h.image.offset, h.image.nbytes, h.image.shape) == (0, n0, 0, ())
	assert (h.uncert.hdu, h.uncert.offset, h.uncert.shape) == (1, n0 + n1, fc.TESS_SHAPE)
	assert h.header['ORIGIN'] == 'primary' and 'TSTART' not in h.header
	# TELESCOP = 'TESS' with another shape is not TESS either
	img = np.zeros((20, 24), dtype='float32')
	p2 = fc.write(tmp_path / 'small.fits', fc.plain_file(img, img, primary_cards=[fc.card('TELESCOP', 'TESS')]))
	h2 = ffi.read_ffi_header(p2)
	assert not h2.is_tess and h2.image.shape == (20, 24) and h2.image.offset == 2880 and h2.uncert.offset == 2 * 2880 + 2880
	assert h2.image.datasum == 0 and h2.uncert.hdu == 1


def test_gz_headers_equal_plain_headers(tmp_path):
	img = np.arange(20 * 24, dtype='float32').reshape(20, 24)
	blob = fc.plain_file(img, img + 1, primary_cards=[fc.card('TSTART', 1.0), fc.card('TSTOP', 2.0)], ext_cards=fc.tan_cards())
	a = ffi.read_ffi_header(fc.write(tmp_path / 'a.fits', blob))
	b = ffi.read_ffi_header(fc.write(tmp_path / 'a.fits.gz', blob))
	assert a[1:] == b[1:]
	assert a.image.datasum == fitsio._sum32(fc.be_bytes(img, -32) + b'\0' * (-img.nbytes % 2880))
	with pytest.raises(ValueError):
		ffi.read_ffi_header(fc.write(tmp_path / 'one.fits', blob[:2880 * 2]))   # a primary HDU alone


def test_ffiindex_extrapolation(tmp_path):
	"""io.py:56-67 by hand: a frame at first_time (with the barycentric correction the reference's numbers imply) is cadence 4697,
	one 1800 s later 4698; the card wins when present; a short exposure gets none."""
	first_time = 0.5 * (1325.317007851970 + 1325.337841177751) - 3.9072474e-03
	assert ffi.extrapolate_ffiindex(1325.317007851970, 1325.337841177751, 3.9072474e-03) == 4697
	assert ffi.extrapolate_ffiindex(first_time - 0.01, first_time + 0.01) == 4697
	step = 1800.0 / 86400.0
	assert ffi.extrapolate_ffiindex(first_time - 0.01 + step, first_time + 0.01 + step) == 4698
	assert ffi.extrapolate_ffiindex(first_time - 0.01 + 100 * step, first_time + 0.01 + 100 * step) == 4797
	assert ffi.extrapolate_ffiindex(first_time + 0.4 * step, first_time + 0.4 * step) == 4697     # rounds to the nearest
	assert ffi.extrapolate_ffiindex(first_time + 0.6 * step, first_time + 0.6 * step) == 4698
	path, *_ = _tess_headers_only(tmp_path, ext=TIME_CARDS)
	assert ffi.read_ffi_header(path).header['FFIINDEX'] == 4697
	later = [fc.card('TSTART', 1325.317007851970 + step), fc.card('TSTOP', 1325.337841177751 + step), fc.card('BARYCORR', 3.9072474e-03), fc.card('EXPOSURE', 0.0165)]
	path, *_ = _tess_headers_only(tmp_path, 'later.fits', ext=later)
	assert ffi.read_ffi_header(path).header['FFIINDEX'] == 4698
	path, *_ = _tess_headers_only(tmp_path, 'card.fits', ext=later + [fc.card('FFIINDEX', 77)])
	assert ffi.read_ffi_header(path).header['FFIINDEX'] == 77
	short = [c for c in later if not c.startswith('EXPOSURE')] + [fc.card('EXPOSURE', 0.001)]           # 86.4 s: not an FFI of 1800 s
	path, *_ = _tess_headers_only(tmp_path, 'short.fits', ext=short)
	assert 'FFIINDEX' not in ffi.read_ffi_header(path).header


def test_find_ffi_files(tmp_path):
	names = {
		'a/tess2018206192942-s0001-1-1-0120-s_ffic.fits': (1, 1, 1),
		'b/tess2018206195942-s0001-1-1-0120-s_ffic.fits.gz': (1, 1, 1),
		'a/tess2018206185942-s0001-1-2-0120-s_ffic.fits': (1, 1, 2),
		'tess2018206202942-s0001-2-1-0120-s_ffic.fits': (1, 2, 1),
		'c/d/tess2018234235942-s0002-1-1-0121-a_ffic.fits': (2, 1, 1),
		'tess2018206192942-s0001-1-1-0120-s_ffir.fits': None,                 # raw, not calibrated
		'tess2018206192942-s0001-1-1-0120-s_ffic.fits.bak': None,
		'tess2018206192942-s001-1-1-0120-s_ffic.fits': None,                  # three-digit sector
		'tess2018206192942-s0001-1-1-0120-q_ffic.fits': None,
		'xtess2018206192942-s0001-1-1-0120-s_ffic.fits': None,
		'tess2018206192942-s0001-123456-0120-s_tp.fits': None,
	}
	for n in names:
		os.makedirs(tmp_path / os.path.dirname(n), exist_ok=True)
		(tmp_path / n).write_bytes(b'')
	def want(sector=None, camera=None, ccd=None):
		keep = [n for n, v in names.items() if v and (sector is None or v[0] == sector) and (camera is None or v[1] == camera) and (ccd is None or v[2] == ccd)]
		return [str(tmp_path / n) for n in sorted(keep, key=os.path.basename)]
	every = ffi.find_ffi_files(str(tmp_path))
	assert every == want() and len(every) == 5
	assert [os.path.basename(f)[:17] for f in every] == ['tess2018206185942', 'tess2018206192942', 'tess2018206195942', 'tess2018206202942', 'tess2018234235942']
	assert ffi.find_ffi_files(str(tmp_path), sector=1) == want(sector=1) and len(want(sector=1)) == 4
	assert ffi.find_ffi_files(str(tmp_path), sector=2) == want(sector=2)
	assert ffi.find_ffi_files(str(tmp_path), sector=3) == []
	assert ffi.find_ffi_files(str(tmp_path), camera=2) == want(camera=2)
	assert ffi.find_ffi_files(str(tmp_path), sector=1, camera=1, ccd=1) == want(1, 1, 1) and len(want(1, 1, 1)) == 2
	assert ffi.find_ffi_files(str(tmp_path), ccd=2) == want(ccd=2)
	assert [ffi.sector_cadence(s) for s in (1, 26, 27, 54, 55, 60)] == [1800, 1800, 600, 600, 200, 200]


def test_fitsio_read_is_unchanged_by_the_shared_card_loop(tmp_path):
	"""``fitsio.read`` gives for a file of ``fitsio``'s own writer what it gave before the card loop moved into ``read_header_blocks``."""
	img = np.arange(12, dtype='float64').reshape(3, 4)
	p = str(tmp_path / 'x.fits')
	fitsio.write(p, [fitsio.primary_hdu([fitsio.card('ORIGIN', "it's"), fitsio.card('NUM', 3), fitsio.card('X', 1.5e-7), fitsio.card('FLAG', True)]),
		fitsio.image_hdu('IMG', img), fitsio.bintable_hdu('TAB', [{'name': 'A', 'format': 'D', 'array': np.arange(5.0)}])])
	hdus = fitsio.read(p)
	assert [sorted(k for k in h if k.startswith('__')) for h, _ in hdus] == [['__checksum_ok__', '__datasum_ok__']] * 3
	assert all(h['__checksum_ok__'] and h['__datasum_ok__'] for h, _ in hdus)
	assert hdus[0][0]['ORIGIN'] == "it's" and hdus[0][0]['NUM'] == 3 and hdus[0][0]['X'] == 1.5e-7 and hdus[0][0]['FLAG'] is True and hdus[0][1] is None
	np.testing.assert_array_equal(hdus[1][1], img)
	np.testing.assert_array_equal(hdus[2][1]['A'], np.arange(5.0))


# ---- fits_rules.h ------------------------------------------------------------------------------------------------------------------
def test_header_compiles_alone(tmp_path):
	src = tmp_path / 'only.cpp'
	src.write_text('#include "fits_rules.h"\nint main() { return tp_fits::item_bytes(-32) - 4; }\n')
	subprocess.run(['g++', '-std=c++17', '-Wall', '-fsyntax-only', '-I' + CSRC, str(src)], check=True)


@pytest.fixture(scope='module')
def driver():
	os.makedirs(OUT_DIR, exist_ok=True)
	subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall', '-I' + CSRC, '-o', OUT, SRC],
		check=True)

	def run(text):
		r = subprocess.run([OUT], input=text, capture_output=True, text=True, timeout=120)
		assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
		assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
		assert r.stderr == '', r.stderr
		assert 'FAILED:' not in r.stdout, r.stdout[-2000:]
		return r.stdout.splitlines()
	return run


def test_item_bytes(driver):
	bitpix = [-32, -64, 8, 16, 32, 64, 0, -16, 4]
	assert driver(f'item {len(bitpix)} ' + ' '.join(map(str, bitpix))) == ['4', '8'] + ['0'] * 7


def _unpack_ok(raw, bitpix, n1, n2, r0, c0, rows, cols, out, pitch):
	"""The argument rules of tp_fits_unpack, restated."""
	return (bitpix in (-32, -64) and 1 <= n1 <= 2**24 and 1 <= n2 <= 2**24 and rows >= 1 and cols >= 1 and r0 >= 0 and c0 >= 0 and r0 + rows <= n2
		and c0 + cols <= n1 and pitch >= cols and raw != 0 and out != 0 and raw % 16 == 0 and out % 4 == 0)


def test_window_check(driver):
	A, B = 0x7f0000000100, 0x7f0000800000
	cases = [
		(A, -32, 2136, 2078, 0, 44, 2048, 2048, B, 2048), (A, -64, 2136, 2078, 0, 44, 2048, 2048, B, 4096), (A, -32, 1, 1, 0, 0, 1, 1, B, 1),
		(A, -32, 13, 7, 2, 3, 5, 9, B, 9), (A, -32, 13, 7, 2, 3, 5, 10, B, 10), (A, -32, 13, 7, 2, 4, 5, 10, B, 10), (A, -32, 13, 7, 2, 3, 6, 9, B, 9),
		(A, -32, 13, 7, 0, 0, 7, 13, B, 13), (A, -32, 13, 7, 0, 0, 8, 13, B, 13), (A, -32, 13, 7, 0, 0, 7, 14, B, 14), (A, -32, 13, 7, -1, 0, 2, 2, B, 2),
		(A, -32, 13, 7, 0, -1, 2, 2, B, 2), (A, -32, 13, 7, 7, 0, 1, 1, B, 1), (A, -32, 13, 7, 0, 13, 1, 1, B, 1), (A, -32, 13, 7, 0, 0, 0, 5, B, 5),
		(A, -32, 13, 7, 0, 0, 5, 0, B, 5), (A, -32, 13, 7, 0, 0, -3, 5, B, 5), (A, -32, 13, 7, 0, 0, 5, 5, B, 4), (A, -32, 13, 7, 0, 0, 5, 5, B, 5),
		(A, 16, 13, 7, 0, 0, 5, 5, B, 5), (A, 32, 13, 7, 0, 0, 5, 5, B, 5), (A, 8, 13, 7, 0, 0, 5, 5, B, 5), (A, 64, 13, 7, 0, 0, 5, 5, B, 5), (A, 0, 13, 7, 0, 0, 5, 5, B, 5),
		(0, -32, 13, 7, 0, 0, 5, 5, B, 5), (A, -32, 13, 7, 0, 0, 5, 5, 0, 5), (A + 4, -32, 13, 7, 0, 0, 5, 5, B, 5), (A + 8, -64, 13, 7, 0, 0, 5, 5, B, 5),
		(A, -32, 13, 7, 0, 0, 5, 5, B + 2, 5), (A, -32, 13, 7, 0, 0, 5, 5, B + 4, 5), (A, -32, 0, 7, 0, 0, 1, 1, B, 1), (A, -32, 2**24, 2**24, 2**24 - 1, 2**24 - 1, 1, 1, B, 1),
		(A, -32, 2**24 + 1, 7, 0, 0, 1, 1, B, 1), (A, -32, 2**31 - 1, 2**31 - 1, 2**31 - 2, 0, 2**31 - 1, 2**31 - 1, B, 2**31 - 1),
	]
	text = f'unpack {len(cases)}\n' + '\n'.join(' '.join(['%x' % c[0]] + [str(v) for v in c[1:8]] + ['%x' % c[8], str(c[9])]) for c in cases)
	out = driver(text)
	want = [_unpack_ok(*c) for c in cases]
	assert [line == 'ok' for line in out] == want
	assert sum(want) >= 9 and want.count(False) >= 20
	assert all(line == 'ok' or line.startswith('refused tp_fits_unpack: ') for line in out)
	assert 'BITPIX' in out[19] and 'leaves the image' in out[5] and out[4] == 'ok'


def _row_plan(raw, item, n1, r0, c0, cols, out, pitch):
	"""The vector / scalar choice restated: the rows move in 16-byte groups when a row of the file and of the output are multiples
	of 16 bytes and the first 16-byte boundary of the output (after `head` values) is one of the file too."""
	if (n1 * item) % 16 or pitch % 4:
		return (0, cols, 0, 0)
	head = next(h for h in range(4) if (out + 4 * h) % 16 == 0)
	if (raw + (r0 * n1 + c0 + head) * item) % 16 or cols - head < 4:
		return (0, cols, 0, 0)
	return (1, head, (cols - head) // 4, (cols - head) % 4)


def test_vector_or_scalar_rows(driver):
	A, B = 0x7f0000000100, 0x7f0000800000
	hand = {
		(A, 4, 2136, 0, 44, 2048, B, 2048): (1, 0, 512, 0),           # the TESS science window: all body
		(A, 8, 2136, 0, 44, 2048, B, 2048): (1, 0, 512, 0),
		(A, 4, 13, 2, 3, 9, B, 9): (0, 9, 0, 0),                      # 7 x 13: rows of 52 bytes
		(A, 4, 16, 0, 4, 8, B, 8): (1, 0, 2, 0),                      # 9 x 16, col0 4, 8 columns
		(A, 4, 16, 0, 4, 11, B, 12): (1, 0, 2, 3),                    # ... 11 columns: body and tail
		(A, 4, 16, 0, 4, 11, B, 11): (0, 11, 0, 0),                   # ... into rows of 44 bytes
		(A, 4, 16, 0, 3, 12, B + 12, 16): (1, 1, 2, 3),               # head, body and tail: the output reaches its boundary where the file does
		(A, 4, 16, 0, 3, 12, B, 16): (0, 12, 0, 0),                   # file and output boundaries disagree
		(A, 4, 16, 0, 4, 3, B, 4): (0, 3, 0, 0),                      # too narrow for a group
		(A, 8, 16, 1, 2, 8, B, 8): (1, 0, 2, 0),
		(A, 8, 16, 1, 1, 8, B, 8): (0, 8, 0, 0),                      # float64 values start on 8-byte boundaries only
		(A, 8, 3, 0, 0, 3, B, 4): (0, 3, 0, 0),
	}
	rng = np.random.default_rng(5)
	cases = list(hand)
	for _ in range(300):
		item = int(rng.choice([4, 8]))
		n1 = 4 * int(rng.integers(1, 10)) if rng.random() < 0.7 else int(rng.integers(1, 40))
		c0 = int(rng.integers(0, n1))
		cols = int(rng.integers(1, n1 - c0 + 1))
		cases.append((A + 16 * int(rng.integers(0, 4)), item, n1, int(rng.integers(0, 5)), c0, cols, B + 4 * int(rng.integers(0, 8)), (cols + 3) // 4 * 4 if rng.random() < 0.7 else cols + int(rng.integers(0, 6))))
	text = f'plan {len(cases)}\n' + '\n'.join(' '.join(['%x' % c[0]] + [str(v) for v in c[1:6]] + ['%x' % c[6], str(c[7])]) for c in cases)
	got = [tuple(int(v) for v in line.split()) for line in driver(text)]
	assert got[:len(hand)] == list(hand.values())
	assert got == [_row_plan(*c) for c in cases]
	assert sum(g[0] for g in got) > 20 and sum(1 for g in got if g[0] and g[1]) > 5      # both paths, heads included
	for g, c in zip(got, cases):
		assert g[1] + 4 * g[2] + g[3] == c[5]                                                  # every column exactly once


def test_float64_conversion_equals_numpy_astype(driver):
	rng = np.random.default_rng(9)
	f32 = np.finfo('float32')
	hand = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1.0 + 2.0**-24, 1.0 + 2.0**-24 + 2.0**-50, 1.0 + 3 * 2.0**-24, float(f32.max), float(f32.max) * (1 + 2.0**-25),
		float(f32.max) * (1 + 2.0**-24), 3.5e38, -3.5e38, 1e300, float(f32.tiny), float(f32.tiny) * (1 - 2.0**-25), float(f32.tiny) / 2, 2.0**-149, 2.0**-150, -2.0**-150,
		2.0**-150 * (1 + 2.0**-52), 3 * 2.0**-150, 2.0**-151, 2.0**-140 * (1 + 2.0**-10), 1e-40, -1e-45, 5e-324, 2.2250738585072014e-308, 1e-310], dtype='float64')
	nan_bits = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0x7ff4000020000000, 0xfff123456789abcd, 0x7fffffffffffffff], dtype='uint64')
	rnd = rng.integers(0, 2**64, size=20000, dtype='uint64')
	near = (rng.normal(size=4000) * 10.0**rng.integers(-46, 40, size=4000)).view('uint64')      # float32's whole range, denormals and overflow included
	with np.errstate(invalid='ignore'):
		ties = (rng.integers(0, 2**32, size=2000, dtype='uint64').astype('uint32').view('float32').astype('float64').view('uint64') | np.uint64(0x10000000))[:2000]
	bits = np.concatenate([hand.view('uint64'), nan_bits, rnd, near, ties])
	out = driver(f'cvt {len(bits)} ' + ' '.join('%016x' % b for b in bits))
	got = np.array([int(line.split()[0], 16) for line in out], dtype='uint32')
	cast = np.array([int(line.split()[1], 16) for line in out], dtype='uint32')
	with np.errstate(over='ignore', under='ignore', invalid='ignore'):
		want = bits.view('float64').astype('float32').view('uint32')
	assert np.array_equal(cast, want)                     # the compiler's own cast agrees with numpy (both are the CPU's conversion)
	bad = np.flatnonzero(got != want)
	assert len(bad) == 0, [('%016x' % bits[i], '%08x' % got[i], '%08x' % want[i]) for i in bad[:10]]
	# the cases are what they claim to be
	w = want.view('float32')
	assert np.any(np.isinf(w[:len(hand)]) & np.isfinite(hand)) and np.any((w != 0) & (np.abs(w) < f32.tiny)) and np.any(np.isnan(w))


def _fold(s):
	while s >> 32:
		s = (s & 0xFFFFFFFF) + (s >> 32)
	return s


def test_carry_fold(driver):
	rng = np.random.default_rng(3)
	sums = [0, 1, 0xFFFFFFFF, 0x100000000, 0x1FFFFFFFE, 0xFFFFFFFF00000000, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF00000001, 0x0001000000000000] + \
		[int(v) for v in rng.integers(0, 2**64, size=200, dtype='uint64')]
	out = driver(f'fold {len(sums)} ' + ' '.join('%x' % s for s in sums))
	assert [int(v, 16) for v in out] == [_fold(s) for s in sums]
	assert all(int(v, 16) < 2**32 for v in out)
	# sums of 0xFFFFFFFF words beyond 2^48, added up one by one: the ones'-complement sum of any number of such words is 0xFFFFFFFF
	cases = [(1, 0xFFFFFFFF), (2, 0xFFFFFFFF), (65537, 0xFFFFFFFF), (70000, 0xFFFFFFFF), (4438800, 0xFFFFFFFF), (70001, 0xFFFFFFFE), (3, 0x80000000), (65536, 0x10000), (0, 5)]
	out = driver(f'wordsum {len(cases)} ' + ' '.join(f'{n} {w:x}' for n, w in cases))
	for line, (n, w) in zip(out, cases):
		s, f = (int(v, 16) for v in line.split())
		assert s == n * w and f == _fold(n * w)
		assert f == (0 if n * w == 0 else (n * w - 1) % 0xFFFFFFFF + 1)          # the closed form of the ones'-complement sum
	assert 70000 * 0xFFFFFFFF > 2**48 and int(out[3].split()[1], 16) == 0xFFFFFFFF
	# the byte-level statement the library's writer uses
	blob = rng.integers(0, 256, size=2880, dtype='uint8').tobytes()
	s = int(np.frombuffer(blob, '>u4').astype('uint64').sum())
	assert int(driver(f'fold 1 {s:x}')[0], 16) == fitsio._sum32(blob) == fc.ones_sum(blob)


def test_datasum_arguments_and_blocks(driver):
	A, S = 0x7f0000000100, 0x7f0000900008
	cases = [(A, 4, S), (A, 2880, S), (A, 17755200, S), (A, 0, S), (0, 0, S), (A, 6, S), (A, 2**34, S), (A, 2**34 - 4, S), (A + 4, 16, S), (A, 16, S + 4), (A, 16, 0), (0, 16, S),
		(A, 16 * 256 * 4, S), (A, 16 * 256 * 4 + 16, S), (A, 16 * 256 * 4 * 2048, S), (A, 16 * 256 * 4 * 5000, S)]
	out = driver(f'datasum {len(cases)} ' + ' '.join(f'{a:x} {n:x} {s:x}' for a, n, s in cases))
	for line, (a, n, s) in zip(out, cases):
		ok = n % 4 == 0 and n < 2**34 and s != 0 and (n == 0 or a != 0) and a % 16 == 0 and s % 8 == 0
		assert line.startswith('ok') == ok, (line, a, n, s)
		if ok:
			assert int(line.split()[1]) == min(max(-(-(n // 16) // 1024), 1), 2048)
