# -*- coding: utf-8 -*-
"""
``tp_deflate`` on the device (csrc/deflate.hip) through ``photometry_amd.deflate``: the case inputs of tests/deflate_common.py as
the streams of one call and of two calls in other orders.  Every stream inflates to its input (zlib), and packed bytes, end offsets
and CRCs are bit-equal to the serial composition of the same rules on the host (tests/hostsim/deflate_rules_host.cpp) and to a second
run; nothing behind the packed total is written; a refused call writes nothing; the gzip members of ``gzip_many`` decompress to their
blobs; the context's allocations are back where they were.
"""
import gzip
import numpy as np
import pytest
import deflate_common as dc

pytestmark = pytest.mark.gpu

C = dc.C


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.fixture(scope='module')
def cases():
	return dc.cases()


@pytest.fixture(scope='module')
def host(cases, tmp_path_factory):
	"""The host driver's result for all cases as one call: computed once."""
	res = dc.host_deflate(tmp_path_factory.mktemp('deflate'), list(cases.values()))
	assert res[0] == 'ok'
	return res


def test_one_call_equals_the_host_composition(ctx, cases, host):
	from photometry_amd import deflate
	assert deflate.chunk_bytes(ctx) == C
	blobs = list(cases.values())
	packed, ends, crcs = deflate.deflate_chunks(ctx, blobs)
	dc.check_streams(blobs, packed, ends, crcs)
	assert np.array_equal(ends, host[2]) and np.array_equal(crcs, host[3])
	assert packed == host[1]
	again = deflate.deflate_chunks(ctx, blobs)                                       # a second run: the same bytes
	assert again[0] == packed and np.array_equal(again[1], ends) and np.array_equal(again[2], crcs)


def test_two_calls_in_other_orders(ctx, cases, host, tmp_path):
	from photometry_amd import deflate
	names = list(cases)
	first, second = names[::-1][:len(names) // 2], names[1::2] + names[0::2][:5]
	for order in (first, second):
		blobs = [cases[n] for n in order]
		packed, ends, crcs = deflate.deflate_chunks(ctx, blobs)
		dc.check_streams(blobs, packed, ends, crcs)
		want = dc.host_deflate(tmp_path, blobs)
		assert packed == want[1] and np.array_equal(ends, want[2]) and np.array_equal(crcs, want[3])


def _raw_call(ctx, blobs, sentinel=0xC7, slack=4096, **how):
	"""``tp_deflate`` by hand over sentinel-filled outputs: ``(rc, out, ends, crcs)`` as host arrays, whole buffers."""
	lib = ctx.lib
	data = np.frombuffer(b''.join(blobs), dtype='uint8')
	offsets = how.get('offsets', dc.offsets_of(blobs))
	n_streams = how.get('n_streams', len(blobs))
	n_chunks = sum(len(dc.chunks_of(b)) for b in blobs)
	bound = sum(int(lib.tp_deflate_bound(len(b))) for b in blobs)
	work_bytes = int(lib.tp_deflate_work_bytes(dc.offsets_of(blobs).ctypes.data, len(blobs)))
	d_in = ctx.array(np.concatenate([data, np.zeros(16, dtype='uint8')]))
	d_out = ctx.array(np.full(bound + slack, sentinel, dtype='uint8'))
	d_end = ctx.array(np.full(n_chunks + 2, 0xC7C7C7C7C7C7C7C7, dtype='uint64'))
	d_crc = ctx.array(np.full(n_chunks + 2, 0xC7C7C7C7, dtype='uint32'))
	d_work = ctx.empty(work_bytes + 16, 'uint8')
	ptr = {'in': d_in.ptr, 'out': d_out.ptr, 'end': d_end.ptr, 'crc': d_crc.ptr, 'work': d_work.ptr}
	for k in how.get('null', ()):
		ptr[k] = None
	for k, step in how.get('misalign', {}).items():
		ptr[k] += step
	rc = lib.tp_deflate(ctx.handle, ptr['in'], None if how.get('null_offsets') else np.ascontiguousarray(offsets, dtype='uint64').ctypes.data, n_streams, ptr['out'],
		how.get('capacity', bound), ptr['end'], ptr['crc'], ptr['work'], how.get('work_bytes', work_bytes))
	ctx.sync()
	return rc, d_out.to_host(), d_end.to_host(), d_crc.to_host(), bound, n_chunks


def test_nothing_behind_the_total_is_written(ctx, cases):
	blobs = [cases[f'random_{C + 1}'], cases[f'zeros_{2 * C + 5}'], cases['far'], cases['one_value']]
	rc, out, ends, crcs, bound, n = _raw_call(ctx, blobs)
	assert rc == 0
	total = int(ends[n - 1])
	assert total <= bound and np.all(out[total:] == 0xC7)                             # the sentinel behind the packed total is intact
	assert np.all(ends[n:] == 0xC7C7C7C7C7C7C7C7) and np.all(crcs[n:] == 0xC7C7C7C7)
	dc.check_streams(blobs, out[:total].tobytes(), ends[:n], crcs[:n])


REFUSALS = [
	('n_streams', dict(n_streams=0), 'n_streams must be at least 1'),
	('null_offsets', dict(null_offsets=True), 'null pointer'),
	('falling_offsets', dict(offsets=[0, 50, 40, 100]), 'must not fall'),
	('total', dict(offsets=[0, 1 << 34], n_streams=1), 'fewer than 2^34 bytes'),
	('null_in', dict(null=['in']), 'null pointer'),
	('null_out', dict(null=['out']), 'null pointer'),
	('null_end', dict(null=['end']), 'null pointer'),
	('null_crc', dict(null=['crc']), 'null pointer'),
	('null_work', dict(null=['work']), 'null pointer'),
	('misaligned_end', dict(misalign={'end': 4}), 'd_chunk_end must be 8-byte aligned'),
	('misaligned_crc', dict(misalign={'crc': 2}), 'd_chunk_crc must be 4-byte aligned'),
	('misaligned_work', dict(misalign={'work': 8}), 'd_work must be 16-byte aligned'),
	('capacity', dict(capacity=109), 'out_capacity is below'),
	('work', dict(work_bytes=2 * (16 + 4 * C + 16400) + 16 - 1), 'work buffer is smaller'),
]


@pytest.mark.parametrize('name,how,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(ctx, name, how, message):
	blobs = [bytes(50), b'', bytes(range(50))]
	rc, out, ends, crcs, _bound, _n = _raw_call(ctx, blobs, **how)
	assert rc == -1                                                                  # TP_ERR_INVALID
	assert message in (ctx.lib.tp_last_error(ctx.handle) or b'').decode()
	assert np.all(out == 0xC7) and np.all(ends == 0xC7C7C7C7C7C7C7C7) and np.all(crcs == 0xC7C7C7C7)


def test_host_only_entries(ctx):
	import zlib
	lib = ctx.lib
	assert [int(lib.tp_deflate_bound(n)) for n in (0, 1, C, C + 1)] == [0, 6, C + 5, C + 11]
	off = np.array([0, 50, 50, 100], dtype='uint64')
	assert int(lib.tp_deflate_work_bytes(off.ctypes.data, 3)) == 2 * (16 + 4 * C + 16400) + 16
	assert int(lib.tp_deflate_work_bytes(off[::-1].copy().ctypes.data, 3)) == 0 and int(lib.tp_deflate_work_bytes(None, 3)) == 0
	a, b = b'light', b' curve'
	assert lib.tp_crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)
	assert lib.tp_crc32_combine(zlib.crc32(a), 0, 0) == zlib.crc32(a) and lib.tp_crc32_combine(0, zlib.crc32(b), len(b)) == zlib.crc32(b)


def test_gzip_many(ctx, cases, monkeypatch):
	from photometry_amd import deflate
	ctx.pinned_trim()
	# every allocation and release on ctx, device and page-locked, counted at the C entries (as tests/test_gpu_tpf_groups.py does)
	live = {'device': 0, 'host': 0}
	lib = ctx.lib
	calls = {name: getattr(lib, name) for name in ('tp_malloc', 'tp_free', 'tp_host_alloc', 'tp_host_free', 'tp_deflate')}
	launches = []

	def counting(name, kind, step):
		def call(handle, *args):
			rc = calls[name](handle, *args)
			if rc == 0 and handle == ctx.handle:
				live[kind] += step
			return rc
		return call
	for name, kind, step in (('tp_malloc', 'device', 1), ('tp_free', 'device', -1), ('tp_host_alloc', 'host', 1), ('tp_host_free', 'host', -1)):
		monkeypatch.setattr(lib, name, counting(name, kind, step))
	monkeypatch.setattr(lib, 'tp_deflate', lambda *args: (launches.append(int(args[3])), calls['tp_deflate'](*args))[1])

	blobs = list(cases.values())
	members = deflate.gzip_many(ctx, blobs)
	assert launches == [len(blobs)]
	assert len(members) == len(blobs)
	for b, m in zip(blobs, members):
		assert gzip.decompress(m) == b
		assert m[:10] == b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff'                   # no FNAME, MTIME = 0, OS = 255
	assert deflate.gzip_many(ctx, blobs) == members                                   # the bytes depend on the content alone
	# an empty blob alone and among others; no blob at all
	(empty,) = deflate.gzip_many(ctx, [b''])
	assert gzip.decompress(empty) == b'' and len(empty) == 20
	assert deflate.gzip_many(ctx, []) == []
	# a batch that max_batch_bytes splits in two: the same members from two calls
	del launches[:]
	some = [cases[f'ramp_{C + 1}'], b'', cases[f'zeros_{C}'], cases['far'], cases[f'random_{260}']]
	split = deflate.gzip_many(ctx, some, max_batch_bytes=2 * C + 1)
	assert launches == [3, 2]                                                        # (C + 1) + 0 + C, then the rest
	assert split == [members[blobs.index(b)] if b else empty for b in some]
	assert live['device'] == 0, live
	ctx.pinned_trim()
	assert live == {'device': 0, 'host': 0}, live
