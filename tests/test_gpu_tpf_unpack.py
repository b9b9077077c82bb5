# -*- coding: utf-8 -*-
"""
The target-pixel-file unpacker on the device through the C ABI (``tp_tpf_unpack``; csrc/tpfin.hip): binary tables built with numpy's
big-endian record dtypes (tests/tpf_common.py), outputs pre-filled with a sentinel and held bit for bit (as ``uint32``) to numpy's
own reading of the same bytes.
"""
import ctypes
import numpy as np
import pytest
import ffi_common as fc
import tpf_common as tc

pytestmark = pytest.mark.gpu

SENTINEL = tc.SENTINEL
GUARD = 64        # sentinel values before and behind every cube: nothing outside [n_pix][t_pitch] may be touched


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _drop(n_rows, gone):
	return [r for r in range(n_rows) if r not in gone]


#: (n_pix, n_rows, kept rows or None, what)
SHAPES = [(1, 1, None, 'smallest'), (3, 5, None, 'odd'), (64, 64, None, 'one full tile'), (65, 65, None, 'one past a tile both ways'),
	(121, 70, None, 'pads 70..95'), (132, 33, None, 'rows of 12 mod 16 bytes'), (121, 200, _drop(200, (0, 99, 100, 199)), 'first, last and two adjacent rows dropped'),
	(625, 130, _drop(130, (64,)), 'one row dropped, ten pixel tiles'), (121, 19000, None, 'the realistic size')]


def _call(ctx, table_ptr, row_bytes, n_rows, rows, T, n_cols, offsets, n_pix, out_ptrs, t_pitch):
	"""``tp_tpf_unpack`` with host arrays built from Python lists (``rows`` / ``offsets`` / ``out_ptrs`` may be None: null pointers)."""
	h_rows = None if rows is None else np.ascontiguousarray(rows, dtype='int32')
	h_offs = None if offsets is None else (ctypes.c_int64 * len(offsets))(*offsets)
	h_outs = None if out_ptrs is None else (ctypes.c_void_p * len(out_ptrs))(*out_ptrs)
	return ctx.lib.tp_tpf_unpack(ctx.handle, table_ptr, row_bytes, n_rows, None if h_rows is None else h_rows.ctypes.data, T, n_cols,
		None if h_offs is None else ctypes.addressof(h_offs), n_pix, None if h_outs is None else ctypes.addressof(h_outs), t_pitch)


def _run(ctx, table, row_bytes, offsets, n_pix, rows, t_pitch=None, shift=0):
	"""Unpack every column of ``table`` (placed ``shift`` bytes past a 256-byte boundary) in one launch; returns the guarded outputs ``(n_cols, GUARD + n_pix * t_pitch + GUARD)``."""
	n_rows = len(table) // row_bytes
	T = n_rows if rows is None else len(rows)
	t_pitch = tc.round_up(T, 32) if t_pitch is None else t_pitch
	host = np.zeros(shift + len(table), dtype='uint8')
	host[shift:] = np.frombuffer(table, dtype='uint8')
	d_table = ctx.array(host)
	assert d_table.ptr % 256 == 0
	n = n_pix * t_pitch
	d_out = ctx.array(np.full((len(offsets), GUARD + n + GUARD), SENTINEL, dtype='uint32'))
	ptrs = [d_out.ptr + 4 * (c * (n + 2 * GUARD) + GUARD) for c in range(len(offsets))]
	rc = _call(ctx, d_table.ptr + shift, row_bytes, n_rows, rows, T, len(offsets), offsets, n_pix, ptrs, t_pitch)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	ctx.sync()
	return d_out.to_host(), T, t_pitch


def _hold(got, table, row_bytes, offsets, n_pix, rows, T, t_pitch, what=''):
	n = n_pix * t_pitch
	for c, off in enumerate(offsets):
		want = tc.expected_cube(table, row_bytes, off, n_pix, rows, t_pitch)
		cube = got[c, GUARD:GUARD + n].reshape(n_pix, t_pitch)
		bad = cube != want
		assert not bad.any(), (what, c, int(bad.sum()), ['%08x %08x' % (a, b) for a, b in zip(cube[bad][:5], want[bad][:5])])
		assert np.all(cube[:, T:] == 0)                                                    # the pad cadences read 0.0
		assert np.all(got[c, :GUARD] == SENTINEL) and np.all(got[c, GUARD + n:] == SENTINEL)   # nothing beyond n_pix * t_pitch is touched


@pytest.mark.parametrize('n_pix,n_rows,rows,what', SHAPES, ids=[s[3] for s in SHAPES])
def test_unpack_equals_numpy(ctx, n_pix, n_rows, rows, what):
	rng = np.random.default_rng(n_pix + n_rows)
	cols = [tc.random_bits((n_rows, n_pix), rng) for _ in range(3)]
	# the rows of a real file: TIME, TIMECORR, CADENCENO and RAW_CNTS ahead of the three columns, FLUX_BKG_ERR, QUALITY and POS_CORR1,2 behind
	table, row_bytes, offsets = tc.bare_table(cols, lead=16 + 4 * n_pix, gaps=(0, 0, 4 * n_pix), trail=12, rng=rng)
	assert row_bytes == 28 + 20 * n_pix
	if n_pix == 132:
		assert row_bytes == 2668 and row_bytes % 16 == 12
	if n_rows == 19000:
		assert 46e6 < len(table) < 47e6
	got, T, t_pitch = _run(ctx, table, row_bytes, offsets, n_pix, rows)
	if (n_pix, n_rows) == (121, 70):
		assert t_pitch == 96
	# a byte swap and nothing else: the planted NaN payloads, signalling NaNs, -0.0 and denormals are among the values
	kept = cols[0] if rows is None else cols[0][rows]
	assert np.array_equal(got[0, GUARD:GUARD + n_pix * t_pitch].reshape(n_pix, t_pitch)[:, :T], kept.T)
	if cols[0].size >= len(tc.PLANT):
		assert set(tc.PLANT.tolist()) <= set(cols[0].ravel().tolist())      # (in the table; a dropped row may hold some of them)
	_hold(got, table, row_bytes, offsets, n_pix, rows, T, t_pitch, what)


@pytest.mark.parametrize('n_cols', [1, 3, 4])
def test_columns_per_launch_and_misaligned_offsets(ctx, n_cols):
	"""One, three and four columns in one launch; lead 20 and gaps of 4 put every column offset on a 4- but not a 16-byte boundary."""
	rng = np.random.default_rng(10 + n_cols)
	n_pix, n_rows = 121, 70
	cols = [tc.random_bits((n_rows, n_pix), rng) for _ in range(n_cols)]
	table, row_bytes, offsets = tc.bare_table(cols, lead=20, gaps=[4] * n_cols, trail=4, rng=rng)
	assert all(o % 4 == 0 and o % 16 != 0 for o in offsets)
	got, T, t_pitch = _run(ctx, table, row_bytes, offsets, n_pix, None)
	_hold(got, table, row_bytes, offsets, n_pix, None, T, t_pitch)
	# the columns in another order, and a pitch well above T: whole tiles of pad cadences
	order = list(reversed(offsets))
	got, T, t_pitch = _run(ctx, table, row_bytes, order, n_pix, None, t_pitch=192)
	_hold(got, table, row_bytes, order, n_pix, None, T, 192)


def test_table_four_bytes_past_a_256_byte_boundary(ctx):
	rng = np.random.default_rng(21)
	n_pix, n_rows = 132, 70
	cols = [tc.random_bits((n_rows, n_pix), rng) for _ in range(3)]
	table, row_bytes, offsets = tc.bare_table(cols, lead=16, trail=12, rng=rng)
	rows = _drop(n_rows, (3,))
	got, T, t_pitch = _run(ctx, table, row_bytes, offsets, n_pix, rows, shift=4)
	_hold(got, table, row_bytes, offsets, n_pix, rows, T, t_pitch)


def test_refused_calls_write_nothing(ctx):
	rng = np.random.default_rng(1)
	n_pix, n_rows, t_pitch = 121, 70, 96
	cols = [tc.random_bits((n_rows, n_pix), rng) for _ in range(3)]
	table, row_bytes, offsets = tc.bare_table(cols, lead=16, trail=12, rng=rng)
	assert row_bytes == 16 + 3 * 484 + 12
	d_table = ctx.array(np.frombuffer(table, dtype='uint8'))
	d_out = ctx.array(np.full((4, n_pix * t_pitch), SENTINEL, dtype='uint32'))
	P = [d_out.ptr + 4 * c * n_pix * t_pitch for c in range(4)]
	good = dict(table=d_table.ptr, row_bytes=row_bytes, n_rows=n_rows, rows=None, T=n_rows, n_cols=3, offsets=offsets, n_pix=n_pix, outs=P[:3], t_pitch=t_pitch)
	refused = [
		(dict(table=None), 'null pointer'), (dict(outs=[P[0], None, P[2]]), 'null pointer'), (dict(offsets=None), 'null pointer'), (dict(outs=None), 'null pointer'),
		(dict(table=d_table.ptr + 2), 'd_table must be 4-byte aligned'), (dict(table=d_table.ptr + 1), '4-byte aligned'),
		(dict(row_bytes=row_bytes + 2), 'row_bytes'), (dict(row_bytes=0), 'row_bytes'),
		(dict(offsets=[offsets[0], offsets[1] + 2, offsets[2]]), 'column offset'), (dict(offsets=[-4, offsets[1], offsets[2]]), 'column offset'),
		(dict(offsets=[offsets[0], offsets[1], offsets[2] + 16]), 'leaves the row'), (dict(n_pix=n_pix + 4), 'leaves the row'),
		(dict(n_cols=0), 'n_cols'), (dict(n_cols=5), 'n_cols'),
		(dict(T=0), 'T must lie'), (dict(T=n_rows + 1), 'T must lie'), (dict(T=n_rows - 1), 'T must equal n_rows'),
		(dict(t_pitch=64), 't_pitch'), (dict(t_pitch=70), 't_pitch'), (dict(t_pitch=100), 't_pitch'),
		(dict(n_rows=2**34 // row_bytes + 1, T=1, rows=[0], t_pitch=32), '2^34'),
		(dict(T=3, rows=[0, 2, 2]), 'increase strictly'), (dict(T=3, rows=[0, 2, 1]), 'increase strictly'), (dict(T=3, rows=[5, 6, n_rows]), 'outside the table'),
		(dict(T=3, rows=[-1, 6, 7]), 'outside the table'),
	]
	for change, fragment in refused:
		a = dict(good)
		a.update(change)
		rc = _call(ctx, a['table'], a['row_bytes'], a['n_rows'], a['rows'], a['T'], a['n_cols'], a['offsets'], a['n_pix'], a['outs'], a['t_pitch'])
		msg = ctx.lib.tp_last_error(ctx.handle).decode()
		assert rc != 0 and msg.startswith('tp_tpf_unpack: ') and fragment in msg, (change, rc, msg)
	ctx.sync()
	assert np.all(d_out.to_host() == SENTINEL)
	# the good call goes through, and the Python layer turns a refusal into the library's usual exception
	a = good
	assert _call(ctx, a['table'], a['row_bytes'], a['n_rows'], a['rows'], a['T'], a['n_cols'], a['offsets'], a['n_pix'], a['outs'], a['t_pitch']) == 0
	ctx.sync()
	got = d_out.to_host()
	assert np.all(got[3] == SENTINEL) and np.array_equal(got[1].reshape(n_pix, t_pitch), tc.expected_cube(table, row_bytes, offsets[1], n_pix, None, t_pitch))
	from photometry_amd._lib import TessphotError
	with pytest.raises(TessphotError, match='n_cols'):
		ctx._check(_call(ctx, a['table'], a['row_bytes'], a['n_rows'], None, a['T'], 7, a['offsets'], a['n_pix'], a['outs'], a['t_pitch']))


def test_table_datasum_equals_the_card_of_the_helper(ctx):
	blob, rec, ap, info = tc.make_tpf(np.random.default_rng(6), 11, 11, 70)
	unit = blob[info['table_offset']:info['table_offset'] + info['table_bytes']]
	card = [blob[i:i + 80] for i in range(0, info['table_offset'], 80) if blob[i:i + 8] == b'DATASUM ']
	assert len(card) == 1 and int(card[0][10:].decode().strip().strip("'")) == info['datasum'] == fc.ones_sum(unit)
	d = ctx.array(np.frombuffer(unit, dtype='uint8'))
	d_sum = ctx.array(np.array([0x5555555555555555], dtype='uint64'))
	ctx._check(ctx.lib.tp_fits_datasum(ctx.handle, d.ptr, len(unit), d_sum.ptr))
	ctx.sync()
	assert int(d_sum.to_host()[0]) == info['datasum']
