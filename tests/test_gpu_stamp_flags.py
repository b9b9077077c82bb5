# -*- coding: utf-8 -*-
"""
The per-stamp flag series on the device through the C ABI (``tp_stamp_flag_series``; csrc/stampflags.hip): stacks, stamps and
expected series of tests/stampflags_common.py, the output pre-filled with a sentinel -- guard values before and behind it and in the
pad ``[T, out_pitch)`` of every row -- and held to ``np.any(flags[:, r1:r2, c1:c2] & bit, axis=(1, 2))`` by exact integer equality.
Every case makes one call.
"""
import numpy as np
import pytest
import stampflags_common as sc

pytestmark = pytest.mark.gpu

TP_ERR_INVALID = -1     # include/tessphot_hip.h
GUARD = 64        # sentinel values before and behind the output: nothing outside [n_targets][out_pitch] may be touched


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _call(ctx, raw, n_frames, R, C, stride, stamps, out_pitch, row0=sc.ROW0, col0=sc.COL0, flag_mask=sc.BIT, out_value=sc.OUT_VALUE, n_targets=None, null=0):
	"""One call of ``tp_stamp_flag_series``: return code and the guarded output ``(GUARD + n * out_pitch + GUARD,)`` as it lies in HBM afterwards."""
	d_flags = ctx.array(np.ascontiguousarray(raw, dtype='uint8'))
	h_stamps = np.ascontiguousarray(stamps, dtype='int64').reshape(-1, 4)
	n = len(h_stamps) if n_targets is None else n_targets
	rows = max(n, len(h_stamps))
	d_out = ctx.array(np.full(GUARD + rows * max(out_pitch, 1) + GUARD, sc.SENTINEL, dtype='int32'))
	rc = ctx.lib.tp_stamp_flag_series(ctx.handle, None if null == 1 else d_flags.ptr, n_frames, R, C, stride, row0, col0, n, None if null == 2 else h_stamps.ctypes.data,
		flag_mask, out_value, None if null == 3 else d_out.ptr + 4 * GUARD, out_pitch)
	ctx.sync()
	got = d_out.to_host()
	d_flags.free()
	d_out.free()
	return rc, got


def _hold(got, want, out_pitch):
	n, T = want.shape
	body = got[GUARD:GUARD + n * out_pitch].reshape(n, out_pitch)
	np.testing.assert_array_equal(body[:, :T], want)
	assert np.all(body[:, T:] == sc.SENTINEL)                                                  # the pad of every row
	assert np.all(got[:GUARD] == sc.SENTINEL) and np.all(got[GUARD + n * out_pitch:] == sc.SENTINEL)


@pytest.mark.parametrize('kind', ['clear', 'other_bits', 'sparse', 'everywhere'])
@pytest.mark.parametrize('pad', [0, 13])
@pytest.mark.parametrize('R,C', sc.REGIONS)
@pytest.mark.parametrize('T', [1, 2, 65])
def test_series_equals_numpy(ctx, T, R, C, pad, kind):
	flags = sc.make_flags(kind, T, R, C, seed=T + R)
	if kind == 'sparse':
		flags[T // 2, R // 2, C // 2] |= sc.BIT          # (at density 1e-3 the small region may hold none)
	raw, stride = sc.with_stride(flags, pad)
	stamps = sc.region_stamps(R, C)
	pitch = T + 3
	rc, got = _call(ctx, raw, T, R, C, stride, sc.to_ccd(stamps), pitch)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	want = sc.expected(flags, [tuple(s) for s in stamps])
	_hold(got, want, pitch)
	assert want.any() == (kind in ('sparse', 'everywhere'))


def test_flagged_pixels_just_outside_a_stamp(ctx):
	flags, stamps = sc.neighbours_case()
	raw, stride = sc.with_stride(flags, 13)
	rc, got = _call(ctx, raw, 10, 40, 130, stride, sc.to_ccd(stamps), 10)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	want = sc.expected(flags, [tuple(s) for s in stamps])
	assert want[0].tolist() == [0] * 9 + [sc.OUT_VALUE] and want[1].tolist() == [sc.OUT_VALUE] * 10
	_hold(got, want, 10)


def test_one_flagged_frame_and_the_first_and_last_pixel_of_a_frame(ctx):
	flags, stamps = sc.single_frames_case()
	raw, stride = sc.with_stride(flags, 0)
	rc, got = _call(ctx, raw, 65, 40, 130, stride, sc.to_ccd(stamps), 65)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	want = sc.expected(flags, [tuple(s) for s in stamps])
	assert [np.flatnonzero(o).tolist() for o in want] == [[16], [31], [64], [16, 31, 64], [], [], [16]]
	_hold(got, want, 65)


def test_a_mask_of_several_bits_and_another_output_value(ctx):
	flags = sc.make_flags('sparse', 5, 5, 7, seed=3)
	raw, stride = sc.with_stride(flags, 0)
	stamps = sc.region_stamps(5, 7)
	rc, got = _call(ctx, raw, 5, 5, 7, stride, sc.to_ccd(stamps), 5, flag_mask=2 | 4 | 0x100, out_value=-7)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	_hold(got, sc.expected(flags, [tuple(s) for s in stamps], bit=6, out_value=-7), 5)


@pytest.mark.parametrize('name', sorted(sc.REFUSALS))
def test_refusals_leave_the_sentinel(ctx, name):
	kw = sc.refusal_base()
	kw.update(sc.REFUSALS[name])
	rc, got = _call(ctx, kw['flags'].ravel(), kw['n_frames'], kw['frame_rows'], kw['frame_cols'], kw['frame_stride'], kw['stamps'], kw['out_pitch'],
		flag_mask=kw['flag_mask'], n_targets=kw.get('n_targets'), null=kw['null'])
	assert rc == TP_ERR_INVALID, (name, rc)
	assert ctx.lib.tp_last_error(ctx.handle).decode().startswith('tp_stamp_flag_series: '), name
	assert np.all(got == sc.SENTINEL), name


def test_the_good_call_of_the_refusals_is_taken(ctx):
	kw = sc.refusal_base()
	rc, got = _call(ctx, kw['flags'].ravel(), 2, 5, 7, 35, kw['stamps'], 3)
	assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
	_hold(got, np.full((2, 2), sc.OUT_VALUE, dtype='int32'), 3)
