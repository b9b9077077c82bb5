# -*- coding: utf-8 -*-
"""
The layout helper and the case tables of tests/test_gpu_frame_layouts.py, checked without a GPU: the three layouts round-trip, poison
and guard positions are exactly the complement of the image, every case satisfies what the C entries require of their geometry
(include/tessphot_hip.h), every buffer reaches as far as the entry's own indexing does, and the references (oracle, scipy, numpy) run
on each case's contiguous array and are finite where the GPU test expects finite values.
"""
import os
import numpy as np
import pytest
import layout_common as lc

ALL_KINDS = ('dense',) + lc.LAYOUTS
SHAPES = [(3, 5, 7), (1, 1, 9), (2, 16, 16), lc.MEDIAN_LAYOUT_SHAPE] + lc.MESH_CASES


@pytest.mark.parametrize('kind', ALL_KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_embed_then_extract_round_trips(kind, shape):
	rng = np.random.default_rng(1)
	for dtype in ('float32', 'float64', 'uint8'):
		a = rng.integers(1, 100, shape).astype(dtype)
		lay = lc.Layout(kind, *shape)
		for fill in (0, 113):
			flat = lay.embed(a, fill)
			assert flat.shape == (lay.size,) and flat.dtype == a.dtype
			np.testing.assert_array_equal(lay.extract(flat), a)
			# everything that is not the image is the fill: the positions are exactly the complement
			mask = lay.image_mask()
			assert int(mask.sum()) == a.size
			assert np.all(flat[~mask] == fill)
			np.testing.assert_array_equal(flat[mask], a.ravel())     # ascending flat position is row-major order of the image


@pytest.mark.parametrize('kind', ALL_KINDS)
def test_poison_and_guard_are_the_complement_of_the_image(kind):
	T, R, C = 2, 6, 10
	lay = lc.Layout(kind, T, R, C)
	a = np.arange(T * R * C, dtype='float32').reshape(T, R, C)
	for poison in lc.POISONS:
		flat = lay.embed(a, poison)
		outside = flat[~lay.image_mask()]
		assert np.all(np.isnan(outside)) if np.isnan(poison) else np.all(outside == np.float32(poison))
		assert np.all(np.isfinite(flat[lay.image_mask()]))
	for dtype in ('float32', 'float64', 'uint8', 'int32'):
		g = lc.guard_buffer(lay, dtype)
		assert lc.guard_intact(lay, g)
		# writing the image keeps the guard; one element beside the image breaks it -- wherever it lies
		g[lay.index().ravel()] = 1
		assert lc.guard_intact(lay, g)
		outside = np.nonzero(~lay.image_mask())[0]
		for pos in (outside[0], outside[len(outside) // 2], outside[-1]):
			h = g.copy()
			h[pos] = 0
			assert not lc.guard_intact(lay, h)
	if kind != 'dense':
		assert int((~lay.image_mask()).sum()) > lc.TAIL          # padding inside the stack, not only the band after it
	flat, n = lc.dense_guarded((3, 4), 'float64')
	assert flat.size == 12 + lc.TAIL and lc.dense_tail_intact(flat, n)
	flat[12] = 0.0
	assert not lc.dense_tail_intact(flat, n)


@pytest.mark.parametrize('kind', ALL_KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_layout_geometry_is_what_the_entries_require(kind, shape):
	"""row_pitch >= frame_cols, frame_stride >= frame_rows * row_pitch (every entry's TP_REQUIRE), and the buffer holds the last element
	``k * frame_stride + r * row_pitch + c`` reaches, with the band behind it."""
	T, R, C = shape
	lay = lc.Layout(kind, T, R, C)
	pitch, stride = lay.args()
	assert pitch >= C and stride >= R * pitch
	reach = lay.offset + (T - 1) * stride + (R - 1) * pitch + (C - 1)
	assert reach == lay.last == int(lay.index().max()) and reach + lc.TAIL < lay.size + 1
	assert lay.offset == int(lay.index().min())
	if kind == 'rows':
		assert pitch == C + 1
	if kind == 'rows13':
		assert pitch == C + 13
	if kind == 'frames':
		assert pitch == C and stride == R * C + 7
	if kind == 'window':
		TT, RR, CC = lay.outer
		assert (pitch, stride) == (CC, RR * CC) and lc.WINDOW_C0 % 4 and lay.offset % 4 and lay.offset == lc.WINDOW_R0 * CC + lc.WINDOW_C0
		assert lc.WINDOW_R0 + R <= RR and lc.WINDOW_C0 + C <= CC and lay.size == TT * RR * CC + lc.TAIL
		# the window as numpy sees it in the larger stack
		a = np.arange(T * R * C, dtype='float64').reshape(T, R, C)
		big = lay.embed(a, -1.0)[:TT * RR * CC].reshape(TT, RR, CC)
		np.testing.assert_array_equal(big[:, lc.WINDOW_R0:lc.WINDOW_R0 + R, lc.WINDOW_C0:lc.WINDOW_C0 + C], a)


def test_cut_cases():
	from oracle import cutout
	paths = set()
	for (T, R, C, H, W, n) in lc.CUT_CASES:
		stamps = lc.cut_stamps(R, C, H, W, n, seed=T)
		assert stamps.shape == (n + 8, 4) and stamps.dtype == np.int32
		assert np.all(stamps[:, 1] - stamps[:, 0] == H) and np.all(stamps[:, 3] - stamps[:, 2] == W)
		paths.add(lc.cut_path(R, C, H, W, len(stamps)))
		# the masked cut picks its path by the same rule
		r0, c0 = stamps[:, 0], stamps[:, 2] - lc.COL_OFFSET
		assert (r0 < 0).any() and (r0 + H > R).any() and (c0 < 0).any() and (c0 + W > C).any()      # out on every side
		assert np.all(r0 + H > 0) and np.all(r0 < R) and np.all(c0 + W > 0) and np.all(c0 < C)      # ... and never clear of the frame
		frames = lc.cut_frames(T, R, C, seed=W)
		for i in (0, len(stamps) - 8, len(stamps) - 1):
			cube = cutout.load_cube(frames, tuple(stamps[i]), 0, lc.COL_OFFSET)
			assert cube.shape == (H, W, T)
			want_nan = np.isnan(lc.crop_expected(np.zeros((R, C)), stamps[i], 0, lc.COL_OFFSET))
			assert np.all(np.isnan(cube[want_nan])) and want_nan.any() == bool(r0[i] < 0 or c0[i] < 0 or r0[i] + H > R or c0[i] + W > C)
	assert paths == {'tiles', 'gather'}
	full = np.arange(12.0).reshape(3, 4)
	np.testing.assert_array_equal(lc.crop_expected(full, (1, 3, 45, 47), 0, 44), full[1:3, 1:3])
	got = lc.crop_expected(full, (-1, 1, 43, 45), 0, 44)
	assert np.isnan(got[0]).all() and np.isnan(got[1, 0]) and got[1, 1] == 0.0


def test_transpose_and_time_cases(golden_dir):
	from oracle import backgrounds as ob, sumimage as osum
	assert any(T % 64 for T, P, tp in lc.TRANSPOSE_CASES) and any(P % 64 for T, P, tp in lc.TRANSPOSE_CASES)
	assert any(tp == T for T, P, tp in lc.TRANSPOSE_CASES) and any(tp > T for T, P, tp in lc.TRANSPOSE_CASES)
	for (T, P, tp) in lc.TRANSPOSE_CASES:
		lay = lc.pixel_layout('frames', T, P)
		assert tp >= T and lay.frame_stride == P + 7 and lay.row_pitch == P
	f, quality = lc.time_frames()
	T, R, C = lc.TIME_CASE
	assert T <= 32 and f.shape == lc.TIME_CASE
	sm = ob.smooth_time(np.moveaxis(f.reshape(T, R * C), 0, -1), 3)
	assert sm.shape == (R * C, T) and np.isnan(sm[3 * C + 4]).all() and np.isfinite(sm[0]).all()
	s = osum.sumimage(np.moveaxis(f, 0, -1), quality)
	assert s.shape == (R, C) and np.isnan(s[3, 4]) and np.isfinite(np.delete(s.ravel(), 3 * C + 4)).all()
	g = np.load(os.path.join(golden_dir, 'golden_shenanigans.npz'))
	assert int(g['n_cases']) >= 1
	for c in range(int(g['n_cases'])):
		ind = g[f's{c}_indicator']
		assert ind.ndim == 3 and ind.dtype == np.float32 and g[f's{c}_mean'].shape == ind.shape[1:] and np.isfinite(g[f's{c}_mean']).all()
		indices = list(range(ind.shape[0]))
		for k in range(0, ind.shape[0], 25):
			own = ob.shenanigans_block_frames(indices, k, 25)
			assert 1 <= len(own) <= 32 and max(own) < ind.shape[0]


def test_median_cases():
	kernels = set()
	for size in lc.MEDIAN_SIZES:
		for (R, C) in lc.MEDIAN_SHAPES:
			kernels.add(lc.median_kernel(size, R, C))
	assert kernels == {'tp_median15_quad_kernel', 'tp_median_filter_kernel<32, true>', 'tp_median_filter_kernel<32, false>'}
	T, R, C = lc.MEDIAN_LAYOUT_SHAPE
	assert {lc.median_kernel(s, R, C) for s in lc.MEDIAN_LAYOUT_SIZES} == kernels            # ... and each of them on every padded layout
	assert all(s % 2 == 1 and s * s <= 256 for s in lc.MEDIAN_SIZES + lc.MEDIAN_LAYOUT_SIZES)
	widths = {C for R, C in lc.MEDIAN_SHAPES}
	assert {31, 33, 127, 129} <= widths and any(R < 9 for R, C in lc.MEDIAN_SHAPES) and any(C < 9 for R, C in lc.MEDIAN_SHAPES)
	img, ref = lc.median_frames(2, 17, 33, seed=3)
	for size in (3, 9, 15):
		for r in (ref, None):
			want = lc.median_expected(img[0], r, size)
			assert want.shape == (17, 33) and want.dtype == np.float32 and np.isfinite(want).mean() > 0.9


def test_flag_cases():
	f, first = lc.flag_frames()
	flags, zero = lc.flag_expected(f, first)
	assert list(zero) == [False, False, True, False]
	assert flags.dtype == np.uint8 and np.all(flags[2] == 3) and flags[1, 0, 50] == 3 and flags[1, 0, 49] == 0 and flags[3, 4, 5] == 1 and flags[3, 6, 7] == 0
	assert flags[0, 3, 10] == 1 and flags[1, 2, 60] == 3


def test_mesh_cases():
	import test_oracle_pins as pins
	from oracle import backgrounds as ob
	for (T, R, C) in lc.MESH_CASES:
		assert R % 64 and C % 64
	T, R, C = lc.MESH_CASES[1]
	f = lc.sky_frames(T, R, C, seed=R)
	ex, sub = lc.exclude_image(R, C), lc.subtract_images(T, R, C)
	assert ex.any() and not ex.all() and sub.dtype == np.float32 and not np.array_equal(sub[0], sub[1])
	for kw in ({}, {'exclude': ex}, {'exclude': np.stack([ex] * T)}, {'subtract': sub}):
		for mesh, nm in lc.mesh_expected(f, **kw):
			assert mesh.shape == nm.shape == (-(-R // 64), -(-C // 64)) and np.isfinite(mesh).any()
	np.testing.assert_array_equal(lc.mesh_expected(f, exclude=ex)[1][0], lc.mesh_expected(f, exclude=np.stack([ex] * T))[1][0])
	bkg, _ = ob.fit_background(f[0])
	assert bkg.shape == (R, C) and np.isfinite(bkg).all()
	for make in (pins.make_ragged_frame, pins.make_second_selection_frame):
		img, expect = make()
		assert img.dtype == np.float32 and np.isfinite(expect)


def test_radial_cases():
	from photometry_amd import prepare
	T, R, C = lc.RADIAL_CASE
	geo = prepare.RadialGeometry((R, C), 1, 1)
	assert geo.n_rings + 4 <= 72 and int(geo.ring_pixels.max()) < R * C and int(geo.ring_offsets[-1]) == len(geo.ring_pixels)
	f = lc.tess_frames(T, R, C, 9, geo.xcen, geo.ycen)
	m = lc.radial_mask(f)
	assert m.any() and not m.all()
	y = lc.ring_profile(geo.bin_center)
	assert y.shape == (T, geo.n_rings)
	for k in range(T):
		ref = lc.radial_expected(y[k], geo.bin_center, 7.5, R, C, geo.xcen, geo.ycen)
		assert ref.shape == (R, C) and np.isfinite(ref).all()
