# -*- coding: utf-8 -*-
"""
The host side of ``ffi.load_ffis(inflate='device')``: the batch size as a pure function, the FFI headers from a ``read(offset, n)``
source held to those from the path, and what the host learns from the front of a ``.gz`` file.  Files from tests/ffi_common.py.
"""
import gzip
import struct
import numpy as np
import pytest
import ffi_common as fc
from photometry_amd import ffi, fitsio, inflate


def test_inflate_batch_files():
	f = ffi.inflate_batch_files
	MB = 1 << 20
	assert f([10 * MB] * 300, [36 * MB] * 300, 200 * 1024 * MB) == 300                     # everything fits: the number of files
	assert f([10 * MB] * 3000, [36 * MB] * 3000, 200 * 1024 * MB) == ffi.INFLATE_BATCH_MAX
	assert f([10 * MB] * 300, [36 * MB] * 300, 2 * 46 * 64 * MB) == 64                      # half of the free memory, 46 MB per file
	assert f([10 * MB, 20 * MB], [36 * MB, 30 * MB], 2 * 56 * 5 * MB, most=4) == 2          # the largest of each kind
	assert f([10 * MB] * 9, [36 * MB] * 9, 2 * 56 * 5 * MB, share=0.25) == 3
	assert f([10 * MB] * 9, [36 * MB] * 9, 0) == 1 and f([10 * MB] * 9, [36 * MB] * 9, -5) == 1   # at least one
	assert f([1], [1], 1 << 30) == 1 and f([0, 0], [0, 0], 1 << 30) == 2                    # sizes round up to 256: no division by zero


def _files(tmp_path):
	rng = np.random.default_rng(3)
	img = rng.normal(100, 5, (20, 24)).astype('float32')
	plain = fc.plain_file(img, np.sqrt(img), primary_cards=[fc.card('TSTART', 1.0), fc.card('TSTOP', 2.0)], ext_cards=fc.tan_cards())
	bits = rng.integers(0, 2**32, size=fc.TESS_SHAPE, dtype='uint64').astype('uint32')
	tess = fc.tess_file(bits, bits, [fc.card('TSTART', 1.0), fc.card('TSTOP', 2.0), fc.card('EXPOSURE', 0.0165), fc.card('FFIINDEX', 4700)], ext_cards=fc.tan_cards())
	return {'plain': (fc.write(tmp_path / 'plain.fits', plain), plain), 'tess': (fc.write(tmp_path / 'tess.fits', tess), tess)}


def test_headers_from_a_source_equal_those_from_the_path(tmp_path):
	for name, (path, blob) in _files(tmp_path).items():
		want = ffi.read_ffi_header(path)
		got = ffi.read_ffi_header_from(path, lambda offset, n: blob[offset:offset + n])
		# a source that holds the whole file still ends with the first data unit; the rest comes through complete_ffi_header
		assert got.path == want.path and got.image == want.image and got.is_tess == want.is_tess and got.uncert is None, name
		if name == 'tess':
			assert got.header == want.header and got.wcs_cards == want.wcs_cards
		else:
			assert got.header == want.header and got.wcs_cards is None
		reads = []
		whole = ffi.complete_ffi_header(got, lambda offset, n: (reads.append(offset), blob[offset:offset + n])[1])
		assert whole == want and min(reads) == want.image.offset + want.image.nbytes       # only header blocks behind the image unit
		# the front alone is enough, and a source that ends early ends the list quietly
		front = blob[:want.image.offset + 100]
		assert ffi.read_ffi_header_from(path, lambda offset, n: front[offset:offset + n]) == got
		assert ffi.complete_ffi_header(got, lambda offset, n: b'') is None
	assert [u[:3] for u in fitsio.scan_hdus_from(lambda o, n: blob[o:o + n], 3)] == [u[:3] for u in fitsio.scan_hdus(path, 3)]


def test_gzip_front(tmp_path, monkeypatch):
	path, blob = _files(tmp_path)['plain']
	gz = fc.write(tmp_path / 'plain.fits.gz', blob)
	front = ffi.gzip_front(gz, 4)
	raw = open(gz, 'rb').read()
	assert (front.size, front.isize, front.crc) == (len(raw), len(blob), struct.unpack('<I', raw[-8:-4])[0]) and front.pitch % 256 == 0 and front.pitch >= len(blob)
	assert front.why_host is None and front.info.image == ffi.read_ffi_header(path).image and raw[front.begin:front.begin + 1] != b'\x1f'
	# `gzip.open` writes the file's name into the header; the same stream behind a header without one, and behind one with a comment too
	assert front.begin == 10 + len('plain.fits') + 1 and raw[3] == inflate.FNAME
	for name, head in (('bare.fits.gz', b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03'), ('more.fits.gz', b'\x1f\x8b\x08\x18\x00\x00\x00\x00\x00\x03a name\x00a comment\x00')):
		other = str(tmp_path / name)
		with open(other, 'wb') as fh:
			fh.write(head + raw[front.begin:])
		assert ffi.gzip_front(other).begin == len(head) and ffi.gzip_front(other).info[1:] == front.info[1:]
	# two members: the last one's ISIZE is smaller than what the headers ask for
	two = str(tmp_path / 'two.fits.gz')
	with open(two, 'wb') as fh:
		fh.write(gzip.compress(blob[:5000], 1) + gzip.compress(blob[5000:], 1))
	assert 'first member ends in the front' in ffi.gzip_front(two).why_host            # (a small file: the front sees the first member's end)
	monkeypatch.setattr(ffi, 'FRONT_INFLATED', fitsio.BLOCK)                           # as for a file whose first member is longer than the front
	assert 'where the headers ask for' in ffi.gzip_front(two).why_host and ffi.gzip_front(gz).why_host is None
	monkeypatch.undo()
	# no gzip member, and a front that does not inflate: InflateError naming the file
	for name, content in (('text.fits.gz', b'not a gzip file, but long enough for a header'), ('broken.fits.gz', raw[:front.begin] + b'\xff' * 40 + raw[-8:])):
		bad = str(tmp_path / name)
		with open(bad, 'wb') as fh:
			fh.write(content)
		with pytest.raises(ffi.InflateError) as e:
			ffi.gzip_front(bad, 7)
		assert bad in str(e.value) and e.value.index == 7 and isinstance(e.value, (ValueError, inflate.InflateError))


def test_load_ffis_refuses_another_inflate():
	with pytest.raises(ValueError, match="'host' or 'device'"):
		ffi.load_ffis(None, ['a.fits'], inflate='gpu')
