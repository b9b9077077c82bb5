# -*- coding: utf-8 -*-
"""
The FITS unpacker on the device through the C ABI (``tp_fits_unpack``, ``tp_fits_datasum``; csrc/fitsin.hip): data units built with
numpy's big-endian types, outputs held bit for bit (as ``uint32``) to numpy's own reading of the same bytes -- ``'>f4'`` viewed
natively, ``'>f8'`` through ``astype('float32')``.
"""
import numpy as np
import pytest
import ffi_common as fc
from photometry_amd import fitsio

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
TESS = (2078, 2136)

#: (image shape, (row0, col0, rows, cols), output pitch, what it exercises)
CASES = [
	((1, 1), (0, 0, 1, 1), 1, 'smallest'),
	((7, 13), (2, 3, 5, 9), 9, 'odd, misaligned: scalar rows'),
	((7, 13), (2, 3, 5, 9), 12, 'the same into padded rows'),
	((9, 16), (0, 4, 9, 8), 8, 'aligned: vector rows'),
	((9, 16), (1, 4, 7, 11), 12, 'vector body and scalar tail'),
	((9, 16), (1, 4, 7, 11), 11, 'the same columns into rows of 44 bytes: scalar rows'),
	((9, 16), (0, 0, 9, 16), 20, 'whole image, padded rows'),
	((5, 1040), (1, 8, 3, 1031), 1032, 'more than one block per row, tail of 3'),
	(TESS, (0, 44, 2048, 2048), 2048, 'TESS geometry'),
]


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _bits(shape, bitpix, rng):
	"""Random bit patterns with NaN (quiet, signalling, payloads), +-inf, -0.0 and denormals planted; for float64 also values that
	round to float32 denormals, to the smallest normal, to infinity, and exact ties."""
	n = int(np.prod(shape))
	if bitpix == -32:
		bits = rng.integers(0, 2**32, size=n, dtype='uint64').astype('uint32')
		plant = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff8abcde, 0x7fffffff, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001, 0x807fffff, 0x00400000,
			0x3f800000], dtype='uint32')
	else:
		bits = rng.integers(0, 2**64, size=n, dtype='uint64')
		if n > 64:
			# half of the values inside float32's range, its denormals and its overflow
			k = n // 2
			bits[:k] = (rng.normal(size=k) * 10.0**rng.integers(-47, 40, size=k)).view('uint64')
		vals = np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, 1e-40, -1e-45, 2.0**-149, 2.0**-150, 3 * 2.0**-150, 2.0**-150 * (1 + 2.0**-52), 2.0**-151, 1.1754943e-38,
			float(np.finfo('float32').tiny) * (1 - 2.0**-25), 3.4028235e38, 3.4028236e38, float(np.finfo('float32').max) * (1 + 2.0**-25), 1e39, -1e300, 5e-324,
			1.0 + 2.0**-24, 1.0 + 3 * 2.0**-24, 1.0 + 2.0**-24 + 2.0**-52], dtype='float64')
		plant = np.concatenate([vals.view('uint64'), np.array([0x7ff0000000000001, 0xfff4000020000000, 0x7ff8000000000000 | 0x123456789, 0xffffffffffffffff], dtype='uint64')])
	where = rng.permutation(n)[:len(plant)]
	bits[where] = plant[:len(where)]
	return bits.reshape(shape)


def _expected(bits, bitpix):
	"""numpy's reading of the big-endian bytes of ``bits``, as uint32."""
	raw = fc.be_bytes(bits, bitpix)
	if bitpix == -32:
		return raw, np.frombuffer(raw, dtype='>f4').reshape(bits.shape).astype('float32').view('uint32')
	with np.errstate(over='ignore', under='ignore', invalid='ignore'):
		return raw, np.frombuffer(raw, dtype='>f8').reshape(bits.shape).astype('float32').view('uint32')


def _unpack(ctx, d_raw, bitpix, shape, window, d_out, pitch):
	r0, c0, rows, cols = window
	return ctx.lib.tp_fits_unpack(ctx.handle, d_raw.ptr, bitpix, shape[1], shape[0], r0, c0, rows, cols, d_out.ptr, pitch)


@pytest.mark.parametrize('bitpix', [-32, -64])
@pytest.mark.parametrize('shape,window,pitch,what', CASES, ids=[c[3] for c in CASES])
def test_unpack_equals_numpy(ctx, bitpix, shape, window, pitch, what):
	rng = np.random.default_rng(abs(bitpix) + shape[1])
	bits = _bits(shape, bitpix, rng)
	raw, want = _expected(bits, bitpix)
	if bitpix == -32:
		assert np.array_equal(want, bits)            # a byte swap and nothing else
	r0, c0, rows, cols = window
	d_raw = ctx.array(np.frombuffer(raw, dtype='uint8'))
	assert d_raw.ptr % 256 == 0
	d_out = ctx.array(np.full((rows, pitch), SENTINEL, dtype='uint32'))
	rc = _unpack(ctx, d_raw, bitpix, shape, window, d_out, pitch)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	ctx.sync()
	got = d_out.to_host()
	bad = got[:, :cols] != want[r0:r0 + rows, c0:c0 + cols]
	assert not bad.any(), (what, int(bad.sum()), ['%08x %08x' % (a, b) for a, b in zip(got[:, :cols][bad][:5], want[r0:r0 + rows, c0:c0 + cols][bad][:5])])
	assert np.all(got[:, cols:] == SENTINEL)         # what lies between two rows is never written


def test_unpack_into_the_middle_of_a_larger_image(ctx):
	"""Head, body and tail: the output starts 12 bytes behind a 16-byte boundary and reaches one where the file does."""
	rng = np.random.default_rng(77)
	for bitpix, shape, window in ((-32, (6, 32), (1, 3, 4, 27)), (-64, (6, 32), (1, 3, 4, 27)), (-32, (6, 32), (0, 2, 6, 30))):
		bits = _bits(shape, bitpix, rng)
		raw, want = _expected(bits, bitpix)
		r0, c0, rows, cols = window
		d_raw = ctx.array(np.frombuffer(raw, dtype='uint8'))
		big = np.full((rows + 2, 40), SENTINEL, dtype='uint32')
		d_big = ctx.array(big)
		off = 40 + c0                                  # row 1, column c0 of the larger image: c0 = 3 is 12 bytes past a boundary
		rc = ctx.lib.tp_fits_unpack(ctx.handle, d_raw.ptr, bitpix, shape[1], shape[0], r0, c0, rows, cols, d_big.ptr + 4 * off, 40)
		assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
		ctx.sync()
		big[1:1 + rows, c0:c0 + cols] = want[r0:r0 + rows, c0:c0 + cols]
		assert np.array_equal(d_big.to_host(), big)


def test_refused_calls_write_nothing(ctx):
	shape = (9, 16)
	bits = _bits(shape, -32, np.random.default_rng(1))
	d_raw = ctx.array(np.frombuffer(fc.be_bytes(bits, -32), dtype='uint8'))
	d_out = ctx.array(np.full((9, 16), SENTINEL, dtype='uint32'))
	refused = [
		(-32, (0, 4, 9, 13), 16), (-32, (1, 0, 9, 4), 16), (-32, (-1, 0, 2, 2), 16), (-32, (0, -4, 2, 8), 16), (-32, (9, 0, 1, 1), 16),      # off the image
		(-32, (0, 0, 0, 4), 16), (-32, (0, 0, 4, 0), 16), (-32, (0, 0, -2, 4), 16),                                                           # no size
		(16, (0, 0, 4, 4), 16), (32, (0, 0, 4, 4), 16), (8, (0, 0, 4, 4), 16), (64, (0, 0, 4, 4), 16),                                         # integer images
		(-32, (0, 0, 4, 8), 4),                                                                                                               # pitch below cols
	]
	for bitpix, window, pitch in refused:
		rc = _unpack(ctx, d_raw, bitpix, shape, window, d_out, pitch)
		msg = ctx.lib.tp_last_error(ctx.handle).decode()
		assert rc != 0 and msg.startswith('tp_fits_unpack: '), (bitpix, window, pitch, rc, msg)
		if bitpix > 0:
			assert 'BITPIX' in msg
	ctx.sync()
	assert np.all(d_out.to_host() == SENTINEL)
	# the Python layer turns the code into the library's usual exception
	from photometry_amd._lib import TessphotError
	with pytest.raises(TessphotError, match='BITPIX'):
		ctx._check(_unpack(ctx, d_raw, 16, shape, (0, 0, 4, 4), d_out, 16))


def _device_sum(ctx, blob):
	d = ctx.array(np.frombuffer(blob, dtype='uint8'))
	d_sum = ctx.array(np.array([0x5555555555555555], dtype='uint64'))
	rc = ctx.lib.tp_fits_datasum(ctx.handle, d.ptr, len(blob), d_sum.ptr)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	ctx.sync()
	return int(d_sum.to_host()[0])


@pytest.mark.parametrize('nbytes', [4, 2880, 17749728])
def test_word_sum_of_random_data(ctx, nbytes):
	blob = np.random.default_rng(nbytes).integers(0, 256, size=nbytes, dtype='uint8').tobytes()
	want = fitsio._sum32(blob)
	assert want == fc.ones_sum(blob)
	assert _device_sum(ctx, blob) == want
	assert _device_sum(ctx, blob) == want           # and again: integer accumulation, the same in every run


def test_word_sum_folds_its_carries(ctx):
	for nbytes in (4, 8, 20, 2880, 4 * 70000, 17749728):
		blob = b'\xff' * nbytes                      # every partial sum carries; the ones'-complement sum of such words is 0xFFFFFFFF
		assert _device_sum(ctx, blob) == 0xFFFFFFFF == fitsio._sum32(blob), nbytes
	assert _device_sum(ctx, b'\0' * 2880) == 0
	assert _device_sum(ctx, b'\x80\0\0\0' * 3 + b'\0\0\0\x01' * 5) == fitsio._sum32(b'\x80\0\0\0' * 3 + b'\0\0\0\x01' * 5) == 0x80000006
	# sizes around the 16-byte pieces and the blocks' shares
	rng = np.random.default_rng(8)
	for nbytes in (12, 16, 28, 16 * 1024 + 4, 16 * 1024 * 4 - 4, 16 * 1024 * 5 + 8):
		blob = rng.integers(0, 256, size=nbytes, dtype='uint8').tobytes()
		assert _device_sum(ctx, blob) == fitsio._sum32(blob), nbytes


def test_word_sum_equals_the_datasum_card_of_the_writer(ctx):
	a = np.random.default_rng(4).normal(size=(37, 53)).astype('float32')
	blob = fitsio.image_hdu('IMG', a)
	hdr_len = 2880
	assert blob[hdr_len - 2880 + 80 * 10:][:3] == b'END'             # the header is one block
	cards = {blob[i:i + 8].decode().strip(): blob[i + 10:i + 80].decode() for i in range(0, hdr_len, 80)}
	card = int(cards['DATASUM'].split('/')[0].strip().strip("'"))
	assert _device_sum(ctx, blob[hdr_len:]) == card
	from photometry_amd._lib import TessphotError
	d, d_sum = ctx.array(np.zeros(16, dtype='uint8')), ctx.array(np.zeros(1, dtype='uint64'))
	with pytest.raises(TessphotError, match='multiple of 4'):
		ctx._check(ctx.lib.tp_fits_datasum(ctx.handle, d.ptr, 6, d_sum.ptr))
