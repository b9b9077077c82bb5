# -*- coding: utf-8 -*-
"""
``tp_inflate`` on the device (csrc/inflate.hip) through ``photometry_amd.inflate``: the case streams of tests/inflate_common.py,
corrupt ones included, as the streams of one call and of a second call in reverse order.  Bytes, statuses, consumed counts and CRCs
equal the composition of the same rules on the host (tests/hostsim/inflate_rules_host.cpp, which runs first, under AddressSanitizer
and UBSan: a stream reaches the device only after the rules have taken it there) and so zlib's verdict; the sentinel bytes around
every slot are intact; a refused call writes nothing; ``gunzip_many`` gives gzip members back, zlib's and the device encoder's own.
"""
import gzip
import struct
import zlib
import numpy as np
import pytest
import inflate_common as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.fixture(scope='module')
def host(tmp_path_factory):
	"""The cases and the host driver's result for them as one call: computed once, before anything goes to the device."""
	tmp = tmp_path_factory.mktemp('inflate')
	cases = ic.cases(tmp)
	res = ic.host_inflate(tmp, [s for s, _ in cases.values()], [n for _, n in cases.values()])
	assert res[0] == 'ok'
	return cases, res


GAP = 5                                                                                  # sentinel bytes between two slots: every slot at another address modulo 4


def _raw_call(ctx, streams, slots, **how):
	"""``tp_inflate`` by hand, the slots ``GAP`` sentinel bytes apart: ``(rc, out, statuses, produced, consumed, crcs, out_offsets)`` as
	host arrays, whole buffers."""
	lib = ctx.lib
	n = how.get('n_streams', len(streams))
	data = np.frombuffer(b''.join(streams) + bytes(16), dtype='uint8')
	in_offsets = np.ascontiguousarray(how.get('in_offsets', ic.offsets_of([len(s) for s in streams])), dtype='uint64')
	# stream s may write [o[s], o[s + 1]): a slot is followed by GAP bytes that belong to no stream when the slots are given as pairs
	begins = np.concatenate([[GAP], GAP + np.cumsum([int(s) + GAP for s in slots])]).astype('uint64')
	out_offsets = np.ascontiguousarray(how.get('out_offsets', begins), dtype='uint64')
	m = len(streams)
	d_in = ctx.array(data)
	d_out = ctx.array(np.full(int(begins[-1]) + 64, ic.SENTINEL, dtype='uint8'))
	d_status = ctx.array(np.full(m + 2, -0x38383839, dtype='int32'))
	d_produced = ctx.array(np.full(m + 2, 0xC7C7C7C7C7C7C7C7, dtype='uint64'))
	d_consumed = ctx.array(np.full(m + 2, 0xC7C7C7C7C7C7C7C7, dtype='uint64'))
	d_crc = ctx.array(np.full(m + 2, 0xC7C7C7C7, dtype='uint32'))
	ptr = {'in': d_in.ptr, 'out': d_out.ptr, 'status': d_status.ptr, 'produced': d_produced.ptr, 'consumed': d_consumed.ptr, 'crc': d_crc.ptr}
	for k in how.get('null', ()):
		ptr[k] = None
	for k, step in how.get('misalign', {}).items():
		ptr[k] += step
	rc = lib.tp_inflate(ctx.handle, ptr['in'], None if how.get('null_in_offsets') else in_offsets.ctypes.data, n, ptr['out'],
		None if how.get('null_out_offsets') else out_offsets.ctypes.data, ptr['status'], ptr['produced'], ptr['consumed'], ptr['crc'])
	ctx.sync()
	got = rc, d_out.to_host(), d_status.to_host(), d_produced.to_host(), d_consumed.to_host(), d_crc.to_host(), begins
	for d in (d_in, d_out, d_status, d_produced, d_consumed, d_crc):
		d.free()
	return got


def test_one_call_equals_the_host_composition(ctx, host):
	from photometry_amd import inflate
	cases, (_, outputs, statuses, produced, consumed, crcs) = host
	got = inflate.inflate_streams(ctx, [s for s, _ in cases.values()], [n for _, n in cases.values()])
	assert np.array_equal(got[1], statuses)
	assert np.array_equal(got[2], consumed) and np.array_equal(got[3], crcs)
	assert got[0] == outputs
	ic.check_against_zlib(cases, got[0], got[1], np.array([len(o) for o in got[0]]), got[2], got[3])


def test_reverse_order_and_sentinels(ctx, host):
	"""The same streams in reverse order, every slot exactly as large as the call may write and GAP sentinel bytes from the next: the
	same per-stream results, and no byte outside the bytes produced is touched."""
	cases, (_, outputs, statuses, produced, consumed, crcs) = host
	names = list(cases)[::-1]
	n = len(names)
	streams, slots = [cases[k][0] for k in names], [cases[k][1] for k in names]
	# slots that are not adjacent: one stream per pair of offsets, the gaps as empty streams' slots would waste them -- so give every
	# stream its slot and every gap to an empty stream that writes nothing
	pairs_streams, pairs_slots = [], []
	for s, size in zip(streams, slots):
		pairs_streams += [s, b'']
		pairs_slots += [size, GAP]
	in_offsets = ic.offsets_of([len(s) for s in pairs_streams])
	out_offsets = GAP + ic.offsets_of(pairs_slots)
	rc, out, st, pr, co, cr, _ = _raw_call(ctx, pairs_streams, slots, in_offsets=in_offsets, out_offsets=out_offsets, n_streams=2 * n)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	st, pr, co, cr = st[:2 * n:2], pr[:2 * n:2], co[:2 * n:2], cr[:2 * n:2]
	back = slice(None, None, -1)
	assert np.array_equal(st, statuses[back]) and np.array_equal(pr, produced[back]) and np.array_equal(co, consumed[back]) and np.array_equal(cr, crcs[back])
	untouched = np.ones(len(out), dtype=bool)
	for k, name in enumerate(names):
		at = int(out_offsets[2 * k])
		assert out[at:at + int(pr[k])].tobytes() == outputs[n - 1 - k], name
		untouched[at:at + int(pr[k])] = False
	assert np.all(out[untouched] == ic.SENTINEL)


REFUSALS = [
	('n_streams', dict(n_streams=0), 'n_streams must be at least 1'),
	('null_in_offsets', dict(null_in_offsets=True), 'null pointer'),
	('null_out_offsets', dict(null_out_offsets=True), 'null pointer'),
	('falling_in_offsets', dict(in_offsets=[0, 2, 1, 4]), 'must not fall'),
	('falling_out_offsets', dict(out_offsets=[0, 20, 10, 40]), 'must not fall'),
	('total_in', dict(in_offsets=[0, 1 << 34], n_streams=1), 'fewer than 2^34 bytes'),
	('total_out', dict(out_offsets=[0, 1 << 34], n_streams=1), 'fewer than 2^34 bytes'),
	('null_in', dict(null=['in']), 'null pointer'),
	('null_out', dict(null=['out']), 'null pointer'),
	('null_status', dict(null=['status']), 'null pointer'),
	('null_produced', dict(null=['produced']), 'null pointer'),
	('null_consumed', dict(null=['consumed']), 'null pointer'),
	('null_crc', dict(null=['crc']), 'null pointer'),
	('misaligned_status', dict(misalign={'status': 2}), 'd_status must be 4-byte aligned'),
	('misaligned_produced', dict(misalign={'produced': 4}), 'd_out_bytes must be 8-byte aligned'),
	('misaligned_consumed', dict(misalign={'consumed': 4}), 'd_in_bytes must be 8-byte aligned'),
	('misaligned_crc', dict(misalign={'crc': 2}), 'd_crc must be 4-byte aligned'),
]


@pytest.mark.parametrize('name,how,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(ctx, name, how, message):
	rc, out, st, pr, co, cr, _ = _raw_call(ctx, [b'\x03\x00', b'', b'\x03\x00'], [10, 10, 10], **how)
	assert rc == -1                                                                  # TP_ERR_INVALID
	assert message in (ctx.lib.tp_last_error(ctx.handle) or b'').decode()
	assert np.all(out == ic.SENTINEL) and np.all(st == -0x38383839) and np.all(pr == 0xC7C7C7C7C7C7C7C7) and np.all(co == 0xC7C7C7C7C7C7C7C7) and np.all(cr == 0xC7C7C7C7)


def _blobs():
	rng = np.random.default_rng(22)
	return [ic.words(rng, 70000), b'', rng.integers(0, 256, 40000, dtype='uint8').tobytes(), bytes(100000), b'x', ic.words(rng, 333)]


def test_gunzip_many_on_gzip_compress(ctx):
	from photometry_amd import inflate
	blobs = _blobs()
	for level in (1, 9):
		assert inflate.gunzip_many(ctx, [gzip.compress(b, level) for b in blobs]) == blobs
	# two calls where max_batch_bytes splits the list
	assert inflate.gunzip_many(ctx, [gzip.compress(b, 6) for b in blobs], max_batch_bytes=150000) == blobs
	assert inflate.gunzip_many(ctx, []) == []


def _member(blob, flags=0, extra=b'', name=b'', comment=b''):
	head = bytearray(b'\x1f\x8b\x08' + bytes([flags]) + b'\x00\x00\x00\x00\x00\x03')
	if flags & 4:
		head += struct.pack('<H', len(extra)) + extra
	if flags & 8:
		head += name + b'\x00'
	if flags & 16:
		head += comment + b'\x00'
	if flags & 2:
		head += struct.pack('<H', zlib.crc32(bytes(head)) & 0xFFFF)
	return bytes(head) + ic.raw(blob, 6) + struct.pack('<II', zlib.crc32(blob), len(blob))


def test_gunzip_many_takes_the_optional_header_fields(ctx):
	from photometry_amd import inflate
	blob = _blobs()[0]
	members = [_member(blob, 4 | 8, extra=b'\x01\x02sub', name=b'tess_ffic.fits'), _member(blob, 2 | 4 | 8 | 16, extra=b'', name=b'n', comment=b'a comment'), _member(blob, 1)]
	assert all(gzip.decompress(m) == blob for m in members)
	assert inflate.gunzip_many(ctx, members) == [blob] * 3


def test_device_round_trip(ctx):
	"""``deflate.gzip_many``'s own members through ``gunzip_many``, and ``gunzip_to_device`` leaves the same bytes on the device."""
	from photometry_amd import deflate, inflate
	blobs = _blobs()
	members = deflate.gzip_many(ctx, blobs)
	assert inflate.gunzip_many(ctx, members) == blobs
	array, offsets = inflate.gunzip_to_device(ctx, members)
	try:
		flat = array.to_host()
		assert [flat[int(a):int(b)].tobytes() for a, b in zip(offsets[:-1], offsets[1:])] == blobs
	finally:
		array.free()


def test_gunzip_many_raises_on_broken_members(ctx):
	from photometry_amd import inflate
	blobs = _blobs()
	good = [gzip.compress(b, 6) for b in blobs]
	flipped = bytearray(good[2])
	flipped[-8] ^= 0x10                                                              # the trailer's CRC
	with pytest.raises(inflate.InflateError) as e:
		inflate.gunzip_many(ctx, good[:2] + [bytes(flipped)] + good[3:])
	assert e.value.index == 2 and e.value.status == 'CRC' and 'member 2' in str(e.value)
	cut = good[0][:len(good[0]) // 2]                                                # a member cut short: its last 8 bytes are no trailer
	with pytest.raises(inflate.InflateError) as e:
		inflate.gunzip_many(ctx, good[1:3] + [cut])
	assert e.value.index == 2 and e.value.status in ('ISIZE', 'INPUT_ENDS', 'OUTPUT_FULL')
	cut = good[0][:-8 - 5] + struct.pack('<II', zlib.crc32(blobs[0]), len(blobs[0]))   # the stream cut short in front of a true trailer
	with pytest.raises(inflate.InflateError) as e:
		inflate.gunzip_many(ctx, [cut])
	assert e.value.index == 0 and e.value.status == 'INPUT_ENDS'
	padded = good[0][:-8] + b'\x00\x00' + good[0][-8:]                               # bytes between the final block and the trailer
	with pytest.raises(inflate.InflateError) as e:
		inflate.gunzip_many(ctx, [padded])
	assert e.value.status == 'TRAILING_BYTES'
	with pytest.raises(inflate.InflateError) as e:
		inflate.gunzip_to_device(ctx, [good[0], b'not a gzip member at all'])
	assert e.value.index == 1 and e.value.status == 'FRAMING'
