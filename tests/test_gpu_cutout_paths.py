# -*- coding: utf-8 -*-
"""
The stamp cutter (csrc/cutout.hip) held to the oracle on every path its launch code picks and at its limits, through the C ABI:
the cases of tests/cutout_common.py (tests/test_cutout_cases_host.py proves, without a GPU, which branch each of them reaches) cut
with tp_cut_stamps, with four stacks in one tp_cut_stamps_multi launch and with tp_cut_stamps_masked; the tile paths against the
gathers on identical stamps; batches that miss the frame altogether; the refusals; tp_crop_sumimage on the same stamps.

The cutter moves bits: every comparison is exact -- the NaN masks are equal and the uint32 views are equal wherever the oracle holds a
number (the frames carry +-inf and -0.0).  Every cube is handed over full of 0xFF bytes (0x7b for the masked entry), so that an element
the cutter forgot shows up, and the padding of the time axis must come back as zeros.
"""
import ctypes
import re
import numpy as np
import pytest
import cutout_common as cc
import layout_common as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _error():
	from photometry_amd._lib import TessphotError
	return TessphotError


def hold(cube, want, T, rows=None, msg=''):
	"""The cube ``(n, H, W, t_pitch)`` against the oracle's ``(n, H, W, T)``; ``rows``: bool ``(n, H, W)``, the pixels to look at."""
	full = cube.data.to_host()
	assert full.shape == want.shape[:3] + (cube.t_pitch,), msg
	sel = slice(None) if rows is None else rows
	got, exp = full[sel], want[sel]
	assert np.all(got[..., T:] == 0), f'{msg}: the padding of the time axis is not zero'
	got = np.ascontiguousarray(got[..., :T])
	nan = np.isnan(exp)
	np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f'{msg}: NaN mask')
	bad = (got.view('uint32') != exp.view('uint32')) & ~nan
	assert not bad.any(), f'{msg}: {int(bad.sum())} elements differ, the first at {tuple(np.argwhere(bad)[0])}'
	return full


def ptrs(items):
	return (ctypes.c_void_p * len(items))(*[x.ptr for x in items])


def new_cubes(ctx, count, n, T, H, W, t_pitch, fill):
	from photometry_amd.device import DeviceCube
	cubes = [DeviceCube(ctx, n, T, H, W, t_pitch=t_pitch) for _ in range(count)]
	for c in cubes:
		c.data.fill_bytes(fill)
	return cubes


def cut(ctx, d_frames, T, R, C, offsets, d_stamps, cubes, d_mask=None, single=False):
	"""One launch on the dense stacks ``d_frames`` into ``cubes``: tp_cut_stamps (``single``), tp_cut_stamps_multi or tp_cut_stamps_masked."""
	desc = cubes[0].desc
	ro, co = offsets
	if single:
		rc = ctx.lib.tp_cut_stamps(ctx.handle, d_frames[0].ptr, T, R, C, C, R * C, ro, co, d_stamps.ptr, ctypes.byref(desc), cubes[0].ptr)
	elif d_mask is None:
		rc = ctx.lib.tp_cut_stamps_multi(ctx.handle, len(d_frames), ptrs(d_frames), T, R, C, C, R * C, ro, co, d_stamps.ptr, ctypes.byref(desc), ptrs(cubes))
	else:
		rc = ctx.lib.tp_cut_stamps_masked(ctx.handle, len(d_frames), ptrs(d_frames), T, R, C, C, R * C, ro, co, d_stamps.ptr, ctypes.byref(desc), d_mask.ptr, ptrs(cubes))
	ctx._check(rc)
	ctx.sync()


def masked_rows_hold(cubes, want, T, mask, msg):
	"""In-mask rows equal the oracle, every other row still carries the fill pattern."""
	m = mask.astype(bool)
	fulls = []
	for k, cube in enumerate(cubes):
		full = hold(cube, want[k], T, rows=m, msg=f'{msg}, stack {k}')
		assert np.all(full[~m].view('uint32') == 0x7b7b7b7b), f'{msg}, stack {k}: a row outside the mask was written'
		fulls.append(full)
	return fulls


@pytest.mark.parametrize('name', list(cc.CASES))
def test_every_case_against_the_oracle(ctx, name):
	c = cc.CASES[name]
	T, R, C, H, W, t_pitch, offsets = c['T'], c['R'], c['C'], c['H'], c['W'], c['t_pitch'], c['offsets']
	stamps = cc.case_stamps(name)
	n = len(stamps)
	facts, mfacts = cc.case_facts(name), cc.case_facts(name, masked=True)
	frames = [cc.make_frames(T, R, C, seed=1000 * k + T + W) for k in range(cc.MAX_STACKS)]
	want = [cc.expected(f, stamps, *offsets) for f in frames]
	d_frames = [ctx.array(f) for f in frames]
	d_stamps = ctx.array(stamps)
	# one stack
	cubes = new_cubes(ctx, 1, n, T, H, W, t_pitch, 255)
	assert cubes[0].t_pitch == facts['t_pitch']
	cut(ctx, d_frames, T, R, C, offsets, d_stamps, cubes, single=True)
	hold(cubes[0], want[0], T, msg=f"{name} ({facts['path']}), tp_cut_stamps")
	# four stacks, one launch
	cubes = new_cubes(ctx, cc.MAX_STACKS, n, T, H, W, t_pitch, 255)
	cut(ctx, d_frames, T, R, C, offsets, d_stamps, cubes)
	for k in range(cc.MAX_STACKS):
		hold(cubes[k], want[k], T, msg=f"{name} ({facts['path']}), tp_cut_stamps_multi, stack {k} of {cc.MAX_STACKS}")
	# masked, two stacks
	mask = cc.case_masks(n, H, W)
	d_mask = ctx.array(mask)
	cubes = new_cubes(ctx, 2, n, T, H, W, t_pitch, 0x7b)
	cut(ctx, d_frames[:2], T, R, C, offsets, d_stamps, cubes, d_mask=d_mask)
	masked_rows_hold(cubes, want, T, mask, f"{name} ({mfacts['path']}), tp_cut_stamps_masked")


@pytest.mark.parametrize('H,W,R,C,n', [(15, 15, 30, 64, 10), (9, 70, 31, 200, 4)])
def test_the_two_paths_cut_the_same_cubes(ctx, H, W, R, C, n):
	"""The same stamps cut from a frame stack on which they are dense (tile paths) and from that stack with rows of other values
	appended below until they are sparse (gathers): no stamp reaches the new rows, so the cubes are the same, bit for bit."""
	T, offsets = 33, (0, lc.COL_OFFSET)
	stamps = cc.make_stamps(R, C, H, W, n, seed=H + W)
	stamps = np.ascontiguousarray(stamps[stamps[:, 1] <= R])       # none that reaches below the frame
	n = len(stamps)
	R2 = R
	while cc.launch_facts(T, R2, C, H, W, n)['path'] != 'gather':
		R2 += 1
	assert cc.launch_facts(T, R, C, H, W, n)['path'] == 'tiles' and cc.launch_facts(T, R, C, H, W, n, masked=True)['path'] == 'tiles_pixels'
	assert cc.launch_facts(T, R2, C, H, W, n, masked=True)['path'] == 'gather' and R2 > R
	small = cc.make_frames(T, R, C, seed=5)
	big = np.concatenate((small, cc.make_frames(T, R2 - R, C, seed=6) + np.float32(100)), axis=1)
	want = cc.expected(small, stamps, *offsets)
	outside = np.all(np.isnan(want), axis=(1, 2, 3))
	assert outside.sum() >= 3 and np.any(np.isnan(want[~outside])) and np.any(~np.isnan(want))
	np.testing.assert_array_equal(cc.expected(big, stamps, *offsets).view('uint32'), want.view('uint32'))
	d_stamps = ctx.array(stamps)
	rng = np.random.default_rng(31)
	mask = (rng.random((n, H, W)) < 0.3).astype('uint8')
	mask[0] = 0
	mask[1] = 1
	d_mask = ctx.array(mask)
	got, got_masked = {}, {}
	for (key, f, rows) in (('tiles', small, R), ('gather', big, R2)):
		d_f = [ctx.array(f)]
		cubes = new_cubes(ctx, 1, n, T, H, W, None, 255)
		cut(ctx, d_f, T, rows, C, offsets, d_stamps, cubes, single=True)
		got[key] = hold(cubes[0], want, T, msg=f'{key} on {rows} rows')
		cubes = new_cubes(ctx, 1, n, T, H, W, None, 0x7b)
		cut(ctx, d_f, T, rows, C, offsets, d_stamps, cubes, d_mask=d_mask)
		got_masked[key] = masked_rows_hold(cubes, [want], T, mask, f'masked {key} on {rows} rows')[0]
	np.testing.assert_array_equal(got['tiles'].view('uint32'), got['gather'].view('uint32'))
	np.testing.assert_array_equal(got_masked['tiles'].view('uint32'), got_masked['gather'].view('uint32'))


@pytest.mark.parametrize('R,C,path', [(30, 30, 'tiles'), (200, 300, 'gather')])
def test_stamps_beyond_the_frame_only(ctx, R, C, path):
	"""A batch in which no stamp touches the frame: no tile list holds anything, the NaN fill alone writes the cubes."""
	T, H, W, offsets = 33, 15, 15, (0, lc.COL_OFFSET)
	stamps = np.ascontiguousarray(cc.make_stamps(R, C, H, W, 1, seed=3)[cc.OUTSIDE])
	n = len(stamps)
	assert n == 4 and cc.launch_facts(T, R, C, H, W, n)['path'] == path
	frames = [cc.make_frames(T, R, C, seed=k) for k in range(2)]
	d_frames = [ctx.array(f) for f in frames]
	d_stamps = ctx.array(stamps)
	want = [cc.expected(f, stamps, *offsets) for f in frames]
	assert all(np.all(np.isnan(w)) for w in want)
	cubes = new_cubes(ctx, 2, n, T, H, W, None, 255)
	cut(ctx, d_frames, T, R, C, offsets, d_stamps, cubes)
	for k in range(2):
		full = hold(cubes[k], want[k], T, msg=f'{path}, stack {k}')
		assert np.all(np.isnan(full[..., :T])) and np.all(full[..., T:] == 0)
	rng = np.random.default_rng(7)
	mask = (rng.random((n, H, W)) < 0.5).astype('uint8')
	mask[2] = 1
	cubes = new_cubes(ctx, 2, n, T, H, W, None, 0x7b)
	d_mask = ctx.array(mask)
	cut(ctx, d_frames, T, R, C, offsets, d_stamps, cubes, d_mask=d_mask)
	masked_rows_hold(cubes, want, T, mask, f'masked {path}')


def test_refusals_leave_the_cube_alone(ctx):
	T, R, C, H, W = 33, 20, 30, 5, 7
	frames = ctx.array(cc.make_frames(T, R, C, seed=1))
	stamps = cc.make_stamps(R, C, H, W, 1, seed=1)
	n = len(stamps)
	d_stamps = ctx.array(stamps)
	d_mask = ctx.array(np.ones((n, H, W), dtype='uint8'))
	lib, h = ctx.lib, ctx.handle

	def refused(message, call, cube):
		with pytest.raises(_error(), match=re.escape(message)):
			ctx._check(call())
		ctx.sync()
		assert np.all(cube.data.to_host().view('uint8') == 0xFF), message

	cube = new_cubes(ctx, 1, n, T, H, W, None, 255)[0]
	desc = cube.desc
	five = (ctypes.c_void_p * 5)(*[frames.ptr] * 5), (ctypes.c_void_p * 5)(*[cube.ptr] * 5)
	stacks = 'tp_cut_stamps: null pointer / 1 .. 4 stacks'
	for count in (5, 0):
		refused(stacks, lambda: lib.tp_cut_stamps_multi(h, count, five[0], T, R, C, C, R * C, 0, 44, d_stamps.ptr, ctypes.byref(desc), five[1]), cube)
		refused(stacks, lambda: lib.tp_cut_stamps_masked(h, count, five[0], T, R, C, C, R * C, 0, 44, d_stamps.ptr, ctypes.byref(desc), d_mask.ptr, five[1]), cube)
	refused('tp_cut_stamps: the cube must have one cadence per frame',
		lambda: lib.tp_cut_stamps(h, frames.ptr, T - 1, R, C, C, R * C, 0, 44, d_stamps.ptr, ctypes.byref(desc), cube.ptr), cube)
	refused('tp_cut_stamps: bad frame geometry',
		lambda: lib.tp_cut_stamps(h, frames.ptr, T, R, C, C - 1, R * C, 0, 44, d_stamps.ptr, ctypes.byref(desc), cube.ptr), cube)
	# one pixel wider than the documented limit: refused on both sides of the density threshold, with and without a mask
	assert cc.launch_facts(T, R, C, 1, 640, 1)['refused'] and cc.launch_facts(T, R, C, 1, 640, 1)['path'] == 'tiles'
	assert cc.launch_facts(T, 200, 300, 1, 640, 1)['refused'] and cc.launch_facts(T, 200, 300, 1, 640, 1)['path'] == 'gather'
	wide = new_cubes(ctx, 1, 1, T, 1, 640, None, 255)[0]
	wdesc = wide.desc
	wmask = ctx.array(np.ones((1, 1, 640), dtype='uint8'))
	big = ctx.array(cc.make_frames(T, 200, 300, seed=2))
	one = (ctypes.c_void_p * 1)(frames.ptr), (ctypes.c_void_p * 1)(big.ptr), (ctypes.c_void_p * 1)(wide.ptr)
	limit = 'tp_cut_stamps: stamp rows wider than 639 pixels are not supported'
	refused(limit, lambda: lib.tp_cut_stamps(h, frames.ptr, T, R, C, C, R * C, 0, 44, d_stamps.ptr, ctypes.byref(wdesc), wide.ptr), wide)
	refused(limit, lambda: lib.tp_cut_stamps(h, big.ptr, T, 200, 300, 300, 200 * 300, 0, 44, d_stamps.ptr, ctypes.byref(wdesc), wide.ptr), wide)
	refused(limit, lambda: lib.tp_cut_stamps_masked(h, 1, one[0], T, R, C, C, R * C, 0, 44, d_stamps.ptr, ctypes.byref(wdesc), wmask.ptr, one[2]), wide)
	refused(limit, lambda: lib.tp_cut_stamps_masked(h, 1, one[1], T, 200, 300, 300, 200 * 300, 0, 44, d_stamps.ptr, ctypes.byref(wdesc), wmask.ptr, one[2]), wide)
	# and the context is none the worse for it: the same cube, cut
	cut(ctx, [frames], T, R, C, (0, 44), d_stamps, [cube], single=True)
	hold(cube, cc.expected(frames.to_host(), stamps, 0, 44), T, msg='after the refusals')


@pytest.mark.parametrize('name', ['g_1x1', 'g_2x65', 't_offsets'])
def test_crop_sumimage_at_the_same_edges(ctx, name):
	"""tp_crop_sumimage on the stamps of the cutter's cases: numpy slicing of the image, NaN outside it -- the wholly-outside stamps, a
	row offset -- and nothing written behind the output."""
	c = cc.CASES[name]
	R, C, H, W = c['R'], c['C'], c['H'], c['W']
	ro, co = c['offsets']
	rng = np.random.default_rng(5)
	full = rng.normal(1000, 30, (R, C))
	full[rng.random((R, C)) < 0.02] = np.nan
	stamps = cc.case_stamps(name)
	n = len(stamps)
	src, d_stamps = ctx.array(full), ctx.array(stamps)
	flat, count = lc.dense_guarded((n, H, W), 'float64')
	out = ctx.array(flat)
	ctx._check(ctx.lib.tp_crop_sumimage(ctx.handle, src.ptr, R, C, C, ro, co, d_stamps.ptr, n, H, W, out.ptr))
	ctx.sync()
	flat = out.to_host()
	assert lc.dense_tail_intact(flat, count), 'the band after the output was written'
	got = flat[:count].reshape(n, H, W)
	for i in range(n):
		np.testing.assert_array_equal(got[i], lc.crop_expected(full, stamps[i], ro, co), err_msg=f'{name}: {stamps[i]}')
	assert np.all(np.isnan(got[cc.OUTSIDE]))
