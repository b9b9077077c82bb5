# -*- coding: utf-8 -*-
"""
Synthetic FFI files for the tests of ``photometry_amd.ffi``, written WITHOUT ``photometry_amd.fitsio``: header cards formatted by
hand, data units from numpy's big-endian types, the DATASUM as the word sum modulo 2^32 - 1 (the closed form of the
ones'-complement sum, not the carry loop the library folds with) -- so that the reader is not held to its own writer.
"""
import gzip
import numpy as np

BLOCK = 2880
TESS_SHAPE = (2078, 2136)


def card(key, value):
	if isinstance(value, bool):
		v = ('T' if value else 'F').rjust(20)
	elif isinstance(value, int):
		v = str(value).rjust(20)
	elif isinstance(value, float):
		v = repr(value).upper()
		if '.' not in v and 'E' not in v:
			v += '.0'
		v = v.rjust(20)
	else:
		v = ("'" + str(value).ljust(8) + "'").ljust(20)
	return (key.ljust(8) + '= ' + v).ljust(80)


def header_bytes(cards):
	txt = ''.join(cards) + 'END'.ljust(80)
	return (txt + ' ' * (-len(txt) % BLOCK)).encode('ascii')


def ones_sum(data):
	"""Ones'-complement sum of the big-endian 32-bit words: for a non-zero sum s, ((s - 1) mod (2^32 - 1)) + 1."""
	s = int(np.frombuffer(data, dtype='>u4').astype(np.uint64).sum())
	return 0 if s == 0 else (s - 1) % 0xFFFFFFFF + 1


def hdu(cards, data=b'', datasum=True):
	data = data + b'\0' * (-len(data) % BLOCK)
	cards = list(cards)
	if datasum:
		cards.append(card('DATASUM', str(ones_sum(data))))
	return header_bytes(cards) + data


def be_bytes(values, bitpix):
	"""The data unit of an array: float32 / float64 values, or their uint32 / uint64 bit patterns, big-endian."""
	a = np.asarray(values)
	code = {(-32, 'f'): '>f4', (-32, 'u'): '>u4', (-64, 'f'): '>f8', (-64, 'u'): '>u8'}[(bitpix, a.dtype.kind)]
	return a.astype(code).tobytes()


def image_cards(first, bitpix, shape):
	return [first, card('BITPIX', bitpix), card('NAXIS', 2), card('NAXIS1', int(shape[1])), card('NAXIS2', int(shape[0]))]


def tan_cards(crval=(120.0, -35.0), crpix=(12.5, 10.5), scale=21.0 / 3600.0, shape=None):
	"""A plain TAN WCS; NAXIS1 / NAXIS2 are those of the HDU it is written into."""
	return [card('WCSAXES', 2), card('CTYPE1', 'RA---TAN'), card('CTYPE2', 'DEC--TAN'), card('CRPIX1', float(crpix[0])), card('CRPIX2', float(crpix[1])),
		card('CRVAL1', float(crval[0])), card('CRVAL2', float(crval[1])), card('CD1_1', -scale), card('CD1_2', 0.0), card('CD2_1', 0.0), card('CD2_2', scale),
		card('CTYPE1P', 'RAWX'), card('CRPIX1P', 1.0)]


def sip_bad_cards():
	"""The 'divergent' header of tests/golden/golden_wcs.npz: a TAN-SIP WCS whose first footprint corner astropy's all_world2pix
	does not bring back (tests/test_gpu_wcs.py holds the device to that), without the cards an image HDU has of its own."""
	import os
	g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_wcs.npz'))
	h = str(g['hdr_strings'][list(g['hdr_names']).index('divergent')])
	cards = [h[i:i + 80] for i in range(0, len(h), 80)]
	return [c for c in cards if c[8:10] == '= ' and c[:8].strip() not in ('NAXIS1', 'NAXIS2')]


def tess_file(image_bits, uncert_bits, time_cards, primary_cards=(), ext_cards=(), datasum=True):
	"""The bytes of a TESS-shaped FFI: primary without data, image and uncertainty extensions (bit patterns uint32 (2078, 2136))."""
	primary = hdu([card('SIMPLE', True), card('BITPIX', 8), card('NAXIS', 0), card('EXTEND', True), card('TELESCOP', 'TESS')] + list(primary_cards), datasum=False)
	ext = []
	for name, bits in (('CAMERA.CCD 1.1 cal', image_bits), ('CAMERA.CCD 1.1 uncert', uncert_bits)):
		cards = image_cards(card('XTENSION', 'IMAGE'), -32, TESS_SHAPE) + [card('PCOUNT', 0), card('GCOUNT', 1), card('EXTNAME', name)]
		if not ext:
			cards += list(time_cards) + list(ext_cards)
		ext.append(hdu(cards, be_bytes(bits, -32), datasum))
	return primary + ext[0] + ext[1]


def plain_file(image, uncert, primary_cards=(), ext_cards=(), bitpix=-32, datasum=True):
	"""The bytes of an FFI that is not from TESS: the image in the primary HDU, the uncertainty in the first extension."""
	shape = np.asarray(image).shape
	primary = hdu(image_cards(card('SIMPLE', True), bitpix, shape) + [card('EXTEND', True)] + list(primary_cards), be_bytes(image, bitpix), datasum)
	ext = hdu(image_cards(card('XTENSION', 'IMAGE'), bitpix, shape) + [card('PCOUNT', 0), card('GCOUNT', 1)] + list(ext_cards), be_bytes(uncert, bitpix), datasum)
	return primary + ext


def write(path, blob):
	if str(path).endswith('.gz'):
		with gzip.open(path, 'wb', compresslevel=1) as fh:
			fh.write(blob)
	else:
		with open(path, 'wb') as fh:
			fh.write(blob)
	return str(path)
