# -*- coding: utf-8 -*-
"""
The frame-stack entries of the C ABI held to the layouts include/tessphot_hip.h promises: every entry that takes ``row_pitch``,
``frame_stride`` or the stride of an image beside the frames is called with padded rows (``rows``: pitch C + 1, ``rows13``: C + 13),
padded frames (``frames``: stride R * C + 7) and on a window of a larger stack (``window``: pointer inside the allocation, pitch the
full width) -- tests/layout_common.py.  Every input element outside the image is poison (NaN in one run, 1e30 in another), every
output element the contract says is not written carries a guard pattern that must come back untouched (row padding, the gap
between frames, a band after the end).  Expected values come from the oracle, scipy or numpy on the contiguous array, at the
tolerances the tests of the contiguous calls use (test_gpu_cutout.py, test_gpu_fullframe.py); and the padded call must equal the
contiguous call bit for bit -- the arithmetic of a pixel does not depend on where it was loaded from.

Which test reaches which median-filter kernel (csrc/background.hip; layout_common.median_kernel restates the choice):
  tp_median15_quad_kernel             test_median_filter_layouts (size 15), test_median_filter_every_kernel (size 15, frames >= 15 x 15)
  tp_median_filter_kernel<32, true>   test_median_filter_layouts (size 11), test_median_filter_every_kernel (9, 11, 13 on frames >= the window)
  tp_median_filter_kernel<32, false>  test_median_filter_layouts (size 5),  test_median_filter_every_kernel (3, 7; 9 .. 15 on the 8-row / 8-column frames)
"""
import ctypes
import os
import numpy as np
import pytest
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


class Buf(object):
	"""A flat host buffer on the device; ``ptr`` points at pixel (0, 0, 0) of the layout (inside the allocation for a window)."""

	def __init__(self, ctx, lay, flat):
		assert flat.shape == (lay.size,)
		self.lay = lay
		self.dev = ctx.array(flat)
		self.ptr = self.dev.ptr + lay.offset * flat.dtype.itemsize

	def image(self):
		"""The image the kernel wrote; asserts that nothing outside it was touched."""
		flat = self.dev.to_host()
		assert lc.guard_intact(self.lay, flat), f'{self.lay.kind}: an element outside the image was written'
		return self.lay.extract(flat)


def put(ctx, lay, array, poison):
	return Buf(ctx, lay, lay.embed(array, poison))


def out(ctx, lay, dtype):
	return Buf(ctx, lay, lc.guard_buffer(lay, dtype))


class DenseOut(object):
	"""A dense output with the guard band behind it."""

	def __init__(self, ctx, shape, dtype):
		flat, self.n = lc.dense_guarded(shape, dtype)
		self.shape = shape
		self.dev = ctx.array(flat)
		self.ptr = self.dev.ptr

	def host(self):
		flat = self.dev.to_host()
		assert lc.dense_tail_intact(flat, self.n), 'the band after a dense output was written'
		return flat[:self.n].reshape(self.shape)


def untouched(dense_out):
	flat = dense_out.dev.to_host()
	return bool(np.all(flat.view('uint8') == 0x7b))


# ---------------------------------------------------------------------------------------------------------------------------------
# stamp cutter
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', lc.POISONS)
@pytest.mark.parametrize('kind', lc.LAYOUTS)
@pytest.mark.parametrize('case', lc.CUT_CASES)
def test_cut_stamps(ctx, case, kind, poison):
	"""tp_cut_stamps, tp_cut_stamps_multi and tp_cut_stamps_masked on padded stacks and on a window of a larger stack, tile-major path
	and per-stamp gather: every cube equals oracle.cutout.load_cube on the contiguous frames -- NaN outside the frame, never the
	poison beside it -- and the masked cut leaves the out-of-mask rows as they were."""
	from oracle import cutout
	from photometry_amd.device import DeviceCube
	T, R, C, H, W, n = case
	frames = [lc.cut_frames(T, R, C, seed=W), lc.cut_frames(T, R, C, seed=W + 1)]
	stamps = lc.cut_stamps(R, C, H, W, n, seed=T)
	n = len(stamps)
	lay = lc.Layout(kind, T, R, C)
	pitch, stride = lay.args()
	bufs = [put(ctx, lay, f, poison) for f in frames]
	d_stamps = ctx.array(stamps)
	want = [np.stack([cutout.load_cube(f, tuple(s), 0, lc.COL_OFFSET) for s in stamps]) for f in frames]

	def check(cube, k, rows=None):
		full = cube.data.to_host()
		assert full.shape == (n, H, W, cube.t_pitch)
		sel = slice(None) if rows is None else rows
		assert np.all(full[sel][..., T:] == 0)
		np.testing.assert_array_equal(full[sel][..., :T], want[k][sel])
		if poison == poison:
			assert not np.any(full == np.float32(poison))
		return full

	# one stack
	cube = DeviceCube(ctx, n, T, H, W)
	cube.data.fill_bytes(255)
	desc = cube.desc
	ctx._check(ctx.lib.tp_cut_stamps(ctx.handle, bufs[0].ptr, T, R, C, pitch, stride, 0, lc.COL_OFFSET, d_stamps.ptr, ctypes.byref(desc), cube.ptr))
	ctx.sync()
	check(cube, 0)
	# two stacks, one launch
	cubes = [DeviceCube(ctx, n, T, H, W) for _ in range(2)]
	for c in cubes:
		c.data.fill_bytes(255)
	fp = (ctypes.c_void_p * 2)(*[b.ptr for b in bufs])
	cp = (ctypes.c_void_p * 2)(*[c.ptr for c in cubes])
	ctx._check(ctx.lib.tp_cut_stamps_multi(ctx.handle, 2, fp, T, R, C, pitch, stride, 0, lc.COL_OFFSET, d_stamps.ptr, ctypes.byref(desc), cp))
	ctx.sync()
	for k in range(2):
		check(cubes[k], k)
	# masked: an empty mask, a full one, random ones -- on the stamps that stick out of the frame too
	rng = np.random.default_rng(23)
	mask = (rng.random((n, H, W)) < 0.16).astype('uint8')
	mask[0] = 0
	mask[1] = 1
	mask[-8:] |= (rng.random((8, H, W)) < 0.5).astype('uint8')
	d_mask = ctx.array(mask)
	for c in cubes:
		c.data.fill_bytes(0x7b)
	ctx._check(ctx.lib.tp_cut_stamps_masked(ctx.handle, 2, fp, T, R, C, pitch, stride, 0, lc.COL_OFFSET, d_stamps.ptr, ctypes.byref(desc), d_mask.ptr, cp))
	ctx.sync()
	m = mask.astype(bool)
	for k in range(2):
		full = check(cubes[k], k, rows=m)
		assert np.all(full[~m].view('uint32') == 0x7b7b7b7b)


@pytest.mark.parametrize('poison', lc.POISONS)
@pytest.mark.parametrize('kind', ('rows', 'rows13', 'window'))
def test_crop_sumimage(ctx, kind, poison):
	"""tp_crop_sumimage with row_pitch > frame_cols: numpy slicing of the contiguous image, NaN outside, the float64 poison never."""
	T, R, C, H, W, n = lc.CUT_CASES[0]
	rng = np.random.default_rng(5)
	full = rng.normal(1000, 30, (R, C))
	full[rng.random((R, C)) < 0.02] = np.nan
	stamps = lc.cut_stamps(R, C, H, W, n, seed=T)
	n = len(stamps)
	lay = lc.Layout(kind, 1, R, C)
	src = put(ctx, lay, full[None], poison)
	d_stamps = ctx.array(stamps)
	got = DenseOut(ctx, (n, H, W), 'float64')
	ctx._check(ctx.lib.tp_crop_sumimage(ctx.handle, src.ptr, R, C, lay.row_pitch, 0, lc.COL_OFFSET, d_stamps.ptr, n, H, W, got.ptr))
	ctx.sync()
	g = got.host()
	for i in range(n):
		np.testing.assert_array_equal(g[i], lc.crop_expected(full, stamps[i], 0, lc.COL_OFFSET), err_msg=str(stamps[i]))
	if poison == poison:
		assert not np.any(g == poison)


# ---------------------------------------------------------------------------------------------------------------------------------
# transpose, smoothing, sum image, block median
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', lc.POISONS)
@pytest.mark.parametrize('case', lc.TRANSPOSE_CASES)
def test_frames_transpose(ctx, case, poison):
	T, P, tp = case
	rng = np.random.default_rng(T + P)
	f = rng.normal(0, 1, (T, 1, P)).astype('float32')
	lay = lc.pixel_layout('frames', T, P)
	src = put(ctx, lay, f, poison)
	got = DenseOut(ctx, (P, tp), 'float32')
	ctx._check(ctx.lib.tp_frames_transpose(ctx.handle, src.ptr, T, P, lay.frame_stride, got.ptr, tp))
	ctx.sync()
	g = got.host()
	np.testing.assert_array_equal(g[:, :T], np.moveaxis(f[:, 0, :], 0, 1))
	assert np.all(g[:, T:] == 0)


@pytest.mark.parametrize('poison', lc.POISONS)
def test_smooth_time_and_sumimage(ctx, poison):
	"""tp_frames_smooth_time (input and output share frame_stride; the gap between the output frames is not written) and
	tp_frames_sumimage with frame_stride > n_pixels: bit for bit the oracle's, like the contiguous calls."""
	from oracle import backgrounds as ob, sumimage as osum
	f, quality = lc.time_frames()
	T, R, C = f.shape
	P = R * C
	lay = lc.pixel_layout('frames', T, P)
	src = put(ctx, lay, f.reshape(T, 1, P), poison)
	dst = out(ctx, lay, 'float32')
	ctx._check(ctx.lib.tp_frames_smooth_time(ctx.handle, T, P, lay.frame_stride, 3, src.ptr, dst.ptr))
	ctx.sync()
	want = np.moveaxis(ob.smooth_time(np.moveaxis(f.reshape(T, P), 0, -1), 3), -1, 0)
	np.testing.assert_array_equal(dst.image()[:, 0, :], want)
	d_quality = ctx.array(quality)
	got = DenseOut(ctx, (R, C), 'float64')
	ctx._check(ctx.lib.tp_frames_sumimage(ctx.handle, T, P, lay.frame_stride, src.ptr, d_quality.ptr, osum.TESS_DEFAULT_BITMASK, got.ptr))
	ctx.sync()
	np.testing.assert_array_equal(got.host(), osum.sumimage(np.moveaxis(f, 0, -1), quality))


@pytest.mark.parametrize('poison', lc.POISONS)
def test_block_median_accumulate(ctx, golden_dir, poison):
	"""tp_frames_block_median_accumulate with frame_stride > n_pixels against the reference's own mean (golden_shenanigans.npz), the
	blocks formed by the oracle's restatement of the reference's shuffle."""
	from oracle import backgrounds as ob
	g = np.load(os.path.join(golden_dir, 'golden_shenanigans.npz'))
	for c in range(int(g['n_cases'])):
		ind = g[f's{c}_indicator']
		T, R, C = ind.shape
		P = R * C
		lay = lc.pixel_layout('frames', T, P)
		src = put(ctx, lay, ind.reshape(T, 1, P), poison)
		flat, n = lc.dense_guarded((R, C), 'float64')
		flat[:n] = 0.0
		acc = ctx.array(flat)
		indices = list(range(T))
		np.random.seed(0)
		np.random.shuffle(indices)
		keep = []
		for k in range(0, T, 25):
			own = ob.shenanigans_block_frames(indices, k, 25)
			idx = ctx.array(np.asarray(own, dtype='int32'))
			keep.append(idx)
			ctx._check(ctx.lib.tp_frames_block_median_accumulate(ctx.handle, src.ptr, P, lay.frame_stride, idx.ptr, len(own), acc.ptr))
		ctx.sync()
		got = acc.to_host()
		assert lc.dense_tail_intact(got, n)
		np.testing.assert_allclose(got[:n].reshape(R, C) / np.ceil(T / 25), g[f's{c}_mean'], rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# median filter
# ---------------------------------------------------------------------------------------------------------------------------------
def _median(ctx, src, lay, T, R, C, d_ref, size, dst):
	ctx._check(ctx.lib.tp_frames_median_filter(ctx.handle, src.ptr, T, R, C, lay.row_pitch, lay.frame_stride, None if d_ref is None else d_ref.ptr, size, dst.ptr))
	ctx.sync()


@pytest.mark.parametrize('poison', lc.POISONS)
@pytest.mark.parametrize('with_ref', (True, False))
@pytest.mark.parametrize('kind', lc.LAYOUTS)
def test_median_filter_layouts(ctx, kind, with_ref, poison):
	"""Each of the three kernels on every layout: the input is read with row_pitch / frame_stride, the reference image is dense, the
	output has the input's layout and nothing between its rows and frames is written; scipy is the check, bit for bit."""
	T, R, C = lc.MEDIAN_LAYOUT_SHAPE
	img, ref = lc.median_frames(T, R, C, seed=21)
	lay = lc.Layout(kind, T, R, C)
	src = put(ctx, lay, img, poison)
	d_ref = ctx.array(ref) if with_ref else None
	for size in lc.MEDIAN_LAYOUT_SIZES:
		dst = out(ctx, lay, 'float32')
		_median(ctx, src, lay, T, R, C, d_ref, size, dst)
		got = dst.image()
		for k in range(T):
			np.testing.assert_array_equal(got[k], lc.median_expected(img[k], ref if with_ref else None, size), err_msg=f'{lc.median_kernel(size, R, C)} size {size} frame {k}')


@pytest.mark.parametrize('size', lc.MEDIAN_SIZES)
def test_median_filter_every_kernel(ctx, size):
	"""Sizes 3 .. 15 on contiguous frames either side of 32 and 128 columns and on frames with one dimension below the window: every
	kernel the entry can pick is held to scipy, bit for bit."""
	for (R, C) in lc.MEDIAN_SHAPES:
		T = 2
		img, ref = lc.median_frames(T, R, C, seed=size + C)
		lay = lc.Layout('dense', T, R, C)
		src = put(ctx, lay, img, np.nan)
		d_ref = ctx.array(ref)
		for r in (d_ref, None):
			dst = out(ctx, lay, 'float32')
			_median(ctx, src, lay, T, R, C, r, size, dst)
			got = dst.image()
			for k in range(T):
				np.testing.assert_array_equal(got[k], lc.median_expected(img[k], ref if r is not None else None, size),
					err_msg=f'{lc.median_kernel(size, R, C)} size {size} on {R} x {C}, frame {k}')


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel flags
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', lc.POISONS)
def test_pixel_flags(ctx, poison):
	"""tp_frames_pixel_flags: padded rows are rejected before anything is written; a padded frame_stride with dense rows gives the
	oracle's flags and zero test -- the all-zero frame sits next to non-zero poison."""
	f, first = lc.flag_frames()
	T, R, C = f.shape
	want_flags, want_zero = lc.flag_expected(f, first)
	d_first = ctx.array(first)
	for kind in ('rows', 'window'):
		lay = lc.Layout(kind, T, R, C)
		src = put(ctx, lay, f, poison)
		flags, zero = DenseOut(ctx, (T, R, C), 'uint8'), DenseOut(ctx, (T,), 'int32')
		with pytest.raises(_error(), match='tp_frames_pixel_flags: frames must be contiguous images'):
			ctx._check(ctx.lib.tp_frames_pixel_flags(ctx.handle, src.ptr, T, R, C, lay.row_pitch, lay.frame_stride, d_first.ptr, 1, 8e4, 1, 2, zero.ptr, flags.ptr))
		ctx.sync()
		assert untouched(flags) and untouched(zero)
	lay = lc.Layout('frames', T, R, C)
	src = put(ctx, lay, f, poison)
	flags, zero = DenseOut(ctx, (T, R, C), 'uint8'), DenseOut(ctx, (T,), 'int32')
	ctx._check(ctx.lib.tp_frames_pixel_flags(ctx.handle, src.ptr, T, R, C, lay.row_pitch, lay.frame_stride, d_first.ptr, 1, 8e4, 1, 2, zero.ptr, flags.ptr))
	ctx.sync()
	np.testing.assert_array_equal(zero.host().astype(bool), want_zero)
	np.testing.assert_array_equal(flags.host(), want_flags)


# ---------------------------------------------------------------------------------------------------------------------------------
# full-frame background: mesh, zoom
# ---------------------------------------------------------------------------------------------------------------------------------
BOX = 64


def _mesh(ctx, src, lay, exclude=None, estride=0, subtract=None, sstride=0, radial=None):
	"""(mesh, nmasked) DenseOuts of tp_background_mesh / tp_background_mesh_radial."""
	T, R, C = lay.T, lay.R, lay.C
	ny, nx = -(-R // BOX), -(-C // BOX)
	mesh, nm = DenseOut(ctx, (T, ny, nx), 'float64'), DenseOut(ctx, (T, ny, nx), 'int32')
	ex = None if exclude is None else exclude.ptr
	if radial is None:
		ctx._check(ctx.lib.tp_background_mesh(ctx.handle, src.ptr, T, R, C, lay.row_pitch, lay.frame_stride, ex, estride,
			None if subtract is None else subtract.ptr, sstride, 8e4, BOX, mesh.ptr, nm.ptr))
	else:
		ctx._check(ctx.lib.tp_background_mesh_radial(ctx.handle, src.ptr, T, R, C, lay.row_pitch, lay.frame_stride, ex, estride,
			ctypes.byref(radial), 8e4, BOX, mesh.ptr, nm.ptr))
	ctx.sync()
	return mesh, nm


class Zoomed(object):
	"""tp_background_mesh_finish on a mesh: the coefficient arrays tp_background_zoom and the _zoom entries take."""

	def __init__(self, ctx, mesh, nm):
		T, ny, nx = mesh.shape
		self.ny, self.nx = ny, nx
		self.coef, self.vmin, self.vmax = ctx.empty((T, ny, nx), 'float64'), ctx.empty((T,), 'float64'), ctx.empty((T,), 'float64')
		ctx._check(ctx.lib.tp_background_mesh_finish(ctx.handle, mesh.ptr, nm.ptr, T, ny, nx, BOX, 50.0, 3, self.coef.ptr, self.vmin.ptr, self.vmax.ptr, None))

	def image(self, ctx, lay):
		dst = out(ctx, lay, 'float32')
		ctx._check(ctx.lib.tp_background_zoom(ctx.handle, self.coef.ptr, self.vmin.ptr, self.vmax.ptr, lay.T, self.ny, self.nx, BOX, lay.R, lay.C,
			lay.row_pitch, lay.frame_stride, dst.ptr))
		ctx.sync()
		return dst.image()

	def spec(self, C):
		from photometry_amd import _lib
		return _lib.tp_zoom_image(self.coef.ptr, self.vmin.ptr, self.vmax.ptr, self.ny, self.nx, BOX, C)


@pytest.mark.parametrize('poison', lc.POISONS)
@pytest.mark.parametrize('kind', lc.LAYOUTS)
@pytest.mark.parametrize('case', lc.MESH_CASES)
def test_background_mesh_and_zoom(ctx, case, kind, poison):
	"""tp_background_mesh and tp_background_zoom on frames that are no multiple of the box: the frames are read with row_pitch /
	frame_stride, the exclude and subtract images stay dense; a shared exclude image (stride 0) against the same image repeated per
	frame; a subtract image per frame.  Mesh and masked counts against the oracle at the tolerances of the contiguous tests
	(counts exact, mesh 1e-9, background 1e-6), and bit for bit against the contiguous call."""
	from oracle import backgrounds as ob
	T, R, C = case
	f = lc.sky_frames(T, R, C, seed=R)
	ex, sub = lc.exclude_image(R, C), lc.subtract_images(T, R, C)
	lay, dense = lc.Layout(kind, T, R, C), lc.Layout('dense', T, R, C)
	src, src0 = put(ctx, lay, f, poison), put(ctx, dense, f, poison)
	d_ex1, d_exT, d_sub = ctx.array(ex), ctx.array(np.stack([ex] * T)), ctx.array(sub)
	variants = {
		'plain': (dict(), dict()),
		'exclude shared': (dict(exclude=d_ex1, estride=0), dict(exclude=ex)),
		'exclude per frame': (dict(exclude=d_exT, estride=R * C), dict(exclude=ex)),
		'subtract per frame': (dict(subtract=d_sub, sstride=R * C), dict(subtract=sub)),
	}
	results = {}
	for name, (kw, okw) in variants.items():
		mesh, nm = _mesh(ctx, src, lay, **kw)
		mesh0, nm0 = _mesh(ctx, src0, dense, **kw)
		m, n = mesh.host(), nm.host()
		np.testing.assert_array_equal(n, nm0.host(), err_msg=name)
		np.testing.assert_array_equal(m, mesh0.host(), err_msg=name)
		for k, (ref_mesh, ref_nm) in enumerate(lc.mesh_expected(f, **okw)):
			np.testing.assert_array_equal(n[k], ref_nm, err_msg=f'{name}, frame {k}')
			np.testing.assert_allclose(m[k], ref_mesh, rtol=1e-9, equal_nan=True, err_msg=f'{name}, frame {k}')
		results[name] = (mesh, nm, m, n)
	np.testing.assert_array_equal(results['exclude shared'][2], results['exclude per frame'][2])
	np.testing.assert_array_equal(results['exclude shared'][3], results['exclude per frame'][3])
	for name, exclude in (('plain', None), ('exclude shared', ex.astype(bool))):
		z = Zoomed(ctx, results[name][0], results[name][1])
		b, b0 = z.image(ctx, lay), z.image(ctx, dense)
		np.testing.assert_array_equal(b, b0, err_msg=name)
		for k in range(T):
			ref, _ = ob.fit_background(f[k], exclude=exclude)
			np.testing.assert_allclose(b[k], ref, rtol=1e-6, err_msg=f'{name}, frame {k}')


@pytest.mark.parametrize('kind', lc.LAYOUTS)
def test_background_hand_cases(ctx, kind):
	"""The hand cases of tests/test_oracle_pins.py (a frame that is no multiple of the box; a cell only the second mesh selection
	rejects) through tp_background_mesh / _finish / _zoom on every layout."""
	import test_oracle_pins as pins
	for make, want_nm, want_mesh in ((pins.make_ragged_frame, [[0, 3712], [1792, 3880]], [[5.0, 1234.0], [9.0, 0.5]]),
			(pins.make_second_selection_frame, [[2050], [0]], [[100.0], [300.0]])):
		img, expect = make()
		R, C = img.shape
		lay = lc.Layout(kind, 1, R, C)
		for poison in lc.POISONS:
			src = put(ctx, lay, img[None], poison)
			mesh, nm = _mesh(ctx, src, lay)
			np.testing.assert_array_equal(nm.host()[0], want_nm)
			np.testing.assert_array_equal(mesh.host()[0], want_mesh)
			np.testing.assert_allclose(Zoomed(ctx, mesh, nm).image(ctx, lay)[0], expect, rtol=1e-7)


def test_background_rejections(ctx):
	"""What the entries refuse: a frame stride below rows * row_pitch (tp_background_zoom used not to look), a mesh that does not
	cover the frame, strides of the dense side images that are neither 0 nor a whole image."""
	T, R, C = 2, 100, 70
	lay = lc.Layout('rows', T, R, C)
	f = lc.sky_frames(T, R, C, seed=1)
	src = put(ctx, lay, f, np.nan)
	mesh, nm = _mesh(ctx, src, lay)
	z = Zoomed(ctx, mesh, nm)
	dst = out(ctx, lay, 'float32')

	def zoom(ny, nx, pitch, stride):
		return ctx.lib.tp_background_zoom(ctx.handle, z.coef.ptr, z.vmin.ptr, z.vmax.ptr, T, ny, nx, BOX, R, C, pitch, stride, dst.ptr)
	with pytest.raises(_error(), match='tp_background_zoom: frame_stride below frame_rows \\* row_pitch'):
		ctx._check(zoom(2, 2, lay.row_pitch, R * lay.row_pitch - 1))
	with pytest.raises(_error(), match='tp_background_zoom: frame_stride below frame_rows \\* row_pitch'):
		ctx._check(zoom(2, 2, lay.row_pitch, R * C))        # the dense stride with padded rows
	with pytest.raises(_error(), match='tp_background_zoom: the mesh does not cover the frame'):
		ctx._check(zoom(1, 2, lay.row_pitch, lay.frame_stride))
	with pytest.raises(_error(), match='tp_background_zoom: bad geometry'):
		ctx._check(zoom(2, 2, C - 1, lay.frame_stride))
	ctx.sync()
	assert np.all(dst.dev.to_host().view('uint8') == 0x7b)
	d_ex, d_sub = ctx.array(np.zeros((T, R, C), dtype='uint8')), ctx.array(np.zeros((T, R, C), dtype='float32'))
	out_mesh, out_nm = DenseOut(ctx, (T, 2, 2), 'float64'), DenseOut(ctx, (T, 2, 2), 'int32')
	for kw, msg in ((dict(ex=d_ex.ptr, es=R * C - 1), 'exclude_frame_stride must be 0 or at least'), (dict(ex=d_ex.ptr, es=-1), 'exclude_frame_stride must be 0 or at least'),
			(dict(sub=d_sub.ptr, ss=lay.row_pitch), 'subtract_frame_stride must be 0 or at least')):
		with pytest.raises(_error(), match=msg):
			ctx._check(ctx.lib.tp_background_mesh(ctx.handle, src.ptr, T, R, C, lay.row_pitch, lay.frame_stride, kw.get('ex'), kw.get('es', 0),
				kw.get('sub'), kw.get('ss', 0), 8e4, BOX, out_mesh.ptr, out_nm.ptr))
	with pytest.raises(_error(), match='tp_background_mesh: bad frame geometry'):
		ctx._check(ctx.lib.tp_background_mesh(ctx.handle, src.ptr, T, R, C, lay.row_pitch, R * C, None, 0, None, 0, 8e4, BOX, out_mesh.ptr, out_nm.ptr))
	ctx.sync()
	assert untouched(out_mesh) and untouched(out_nm)


# ---------------------------------------------------------------------------------------------------------------------------------
# radial component
# ---------------------------------------------------------------------------------------------------------------------------------
def _bw_constant():
	# kernels.Gaussian().normal_reference_constant of statsmodels
	c = np.pi**0.5 * 2.0**3 * (1.0 / (2.0 * np.sqrt(np.pi))) / (2 * 2 * 24.0)
	return 2 * c**(1.0 / 5)


class Radial(object):
	"""The small arrays of the radial entries for one geometry."""

	def __init__(self, ctx, T, R, C):
		from photometry_amd import prepare
		self.ctx, self.T, self.R, self.C, self.P = ctx, T, R, C, R * C
		self.geo = geo = prepare.RadialGeometry((R, C), 1, 1)
		self.d_pixels, self.d_offsets = ctx.array(geo.ring_pixels), ctx.array(geo.ring_offsets)
		self.n_ring_pixels = int(geo.ring_offsets[-1])
		self.n_partial = 256
		self.d_partial = ctx.empty((T, self.n_partial), 'float64')
		self.d_scratch = ctx.empty((T, self.n_ring_pixels), 'float64')

	def zeropoint(self, src, stride, square=None, sqstride=0, zoom=None, exclude=None, estride=0):
		ctx, lib = self.ctx, self.ctx.lib
		zp = DenseOut(ctx, (self.T,), 'float64')
		ex = None if exclude is None else exclude.ptr
		if zoom is None:
			ctx._check(lib.tp_radial_zeropoint(ctx.handle, src.ptr, self.T, self.P, stride, None if square is None else square.ptr, sqstride, ex, estride, 8e4,
				self.d_partial.ptr, self.n_partial, zp.ptr))
		else:
			ctx._check(lib.tp_radial_zeropoint_zoom(ctx.handle, src.ptr, self.T, self.P, stride, ctypes.byref(zoom), ex, estride, 8e4,
				self.d_partial.ptr, self.n_partial, zp.ptr))
		ctx.sync()
		return zp

	def ring_modes(self, src, stride, zp, square=None, sqstride=0, zoom=None, exclude=None, estride=0):
		ctx, lib, geo = self.ctx, self.ctx.lib, self.geo
		modes, counts = DenseOut(ctx, (self.T, geo.n_rings), 'float64'), DenseOut(ctx, (self.T, geo.n_rings), 'int32')
		ex = None if exclude is None else exclude.ptr
		tail = (zp.ptr, self.d_pixels.ptr, self.d_offsets.ptr, geo.n_rings, self.n_ring_pixels, _bw_constant(), self.d_scratch.ptr, modes.ptr, counts.ptr)
		if zoom is None:
			ctx._check(lib.tp_radial_ring_modes(ctx.handle, src.ptr, self.T, self.P, stride, None if square is None else square.ptr, sqstride, ex, estride, 8e4, *tail))
		else:
			ctx._check(lib.tp_radial_ring_modes_zoom(ctx.handle, src.ptr, self.T, self.P, stride, ctypes.byref(zoom), ex, estride, 8e4, *tail))
		ctx.sync()
		return modes.host(), counts.host()

	def ring_counts(self, mask):
		geo = self.geo
		return np.array([[np.sum(~mask[k].ravel()[geo.ring_pixels[a:b]]) for a, b in zip(geo.ring_offsets[:-1], geo.ring_offsets[1:])] for k in range(self.T)])


@pytest.mark.parametrize('poison', lc.POISONS)
def test_radial_zeropoint_and_ring_modes(ctx, poison):
	"""tp_radial_zeropoint / tp_radial_ring_modes and their _zoom forms with frame_stride > n_pixels, a square image per frame with a
	padded stride of its own, the exclude image shared (stride 0) against repeated per frame: zero point and ring counts against
	numpy (exact), the implicit square component equal to the stored one, padded equal to contiguous, all bit for bit."""
	T, R, C = lc.RADIAL_CASE
	P = R * C
	rad = Radial(ctx, T, R, C)
	f = lc.tess_frames(T, R, C, 9, rad.geo.xcen, rad.geo.ycen)
	ex = lc.exclude_image(R, C)
	lay, dense = lc.pixel_layout('frames', T, P), lc.pixel_layout('dense', T, P)
	src, src0 = put(ctx, lay, f.reshape(T, 1, P), poison), put(ctx, dense, f.reshape(T, 1, P), poison)
	d_ex1, d_exT = ctx.array(ex), ctx.array(np.stack([ex] * T))
	# ---- first iteration: no square component
	for exclude, variants in ((None, [dict()]), (ex, [dict(exclude=d_ex1, estride=0), dict(exclude=d_exT, estride=P)])):
		mask = lc.radial_mask(f, exclude)
		want_zp = np.array([-np.float64(f[k][~mask[k]].min()) + 1.0 for k in range(T)])
		want_counts = rad.ring_counts(mask)
		first = None
		for kw in variants:
			zp, zp0 = rad.zeropoint(src, lay.frame_stride, **kw), rad.zeropoint(src0, P, **kw)
			np.testing.assert_array_equal(zp.host(), want_zp)
			np.testing.assert_array_equal(zp0.host(), want_zp)
			modes, counts = rad.ring_modes(src, lay.frame_stride, zp, **kw)
			modes0, counts0 = rad.ring_modes(src0, P, zp0, **kw)
			np.testing.assert_array_equal(counts, want_counts)
			np.testing.assert_array_equal(counts0, want_counts)
			np.testing.assert_array_equal(modes, modes0)
			assert np.isfinite(modes).sum() >= 30
			if first is not None:
				np.testing.assert_array_equal(modes, first)        # shared exclude image == the same image per frame
			first = modes
	# ---- later iterations: the square component stored (per frame, its own padded stride) and implicit (tp_zoom_image)
	dlay = lc.Layout('dense', T, R, C)
	mesh, nm = _mesh(ctx, put(ctx, dlay, f, poison), dlay)
	z = Zoomed(ctx, mesh, nm)
	square = z.image(ctx, dlay)
	assert np.isfinite(square).all()
	sqlay = lc.pixel_layout('frames', T, P, frame_pad=5)
	d_sq, d_sq0 = put(ctx, sqlay, square.reshape(T, 1, P), poison), put(ctx, dense, square.reshape(T, 1, P), poison)
	zoom = z.spec(C)
	mask = lc.radial_mask(f, ex)
	want_zp = np.array([-np.min((f[k].astype('float64') - square[k].astype('float64'))[~mask[k]]) + 1.0 for k in range(T)])
	want_counts = rad.ring_counts(mask)
	got = []
	for s, stride in ((src, lay.frame_stride), (src0, P)):
		for kw in (dict(square=d_sq, sqstride=sqlay.frame_stride), dict(square=d_sq0, sqstride=P), dict(zoom=zoom)):
			for ekw in (dict(exclude=d_ex1, estride=0), dict(exclude=d_exT, estride=P)):
				zp = rad.zeropoint(s, stride, **kw, **ekw)
				np.testing.assert_array_equal(zp.host(), want_zp)
				modes, counts = rad.ring_modes(s, stride, zp, **kw, **ekw)
				np.testing.assert_array_equal(counts, want_counts)
				got.append(modes)
	assert np.isfinite(got[0]).sum() >= 30
	for m in got[1:]:
		np.testing.assert_array_equal(m, got[0])
	# ---- strides of the side images that are neither 0 nor a whole image
	for kw, msg in ((dict(square=d_sq0, sqstride=P - 1), 'square_frame_stride must be 0 or at least n_pixels'), (dict(exclude=d_exT, estride=1), 'exclude_frame_stride must be 0 or at least n_pixels')):
		with pytest.raises(_error(), match='tp_radial_zeropoint: ' + msg):
			rad.zeropoint(src, lay.frame_stride, **kw)
		with pytest.raises(_error(), match='tp_radial_ring_modes: ' + msg):
			rad.ring_modes(src, lay.frame_stride, zp, **kw)
	with pytest.raises(_error(), match='tp_radial_zeropoint: bad frame geometry'):
		rad.zeropoint(src, P - 1)


@pytest.mark.parametrize('poison', lc.POISONS)
def test_radial_evaluate_and_mesh_radial(ctx, poison):
	"""tp_radial_evaluate / _evaluate_zoom with a padded output stride and d_add per frame on a stride of its own: against scipy at
	the tolerance of test_gpu_fullframe.py::test_radial_pieces, the gap between the output frames untouched, implicit == stored and
	padded == contiguous bit for bit.  tp_background_mesh_radial on every layout: equal to tp_background_mesh with the stored radial
	image as d_subtract (bit for bit), which is held to the oracle at the contiguous test's tolerances."""
	from photometry_amd import prepare, _lib
	T, R, C = lc.RADIAL_CASE
	P = R * C
	rad = Radial(ctx, T, R, C)
	geo = rad.geo
	f = lc.tess_frames(T, R, C, 9, geo.xcen, geo.ycen)
	y = lc.ring_profile(geo.bin_center)
	knots, coefs, nk = prepare.radial_profiles(y, geo.bin_center, radial_smooth=0)
	K = knots.shape[1]
	zps = np.array([7.5, 3.25])
	dk, dc, dn, dzp = ctx.array(knots), ctx.array(coefs), ctx.array(nk), ctx.array(zps)
	want = np.stack([lc.radial_expected(y[k], geo.bin_center, zps[k], R, C, geo.xcen, geo.ycen) for k in range(T)])
	spec = _lib.tp_radial_image(float(lc.COL_OFFSET), float(geo.xcen), float(geo.ycen), dk.ptr, dc.ptr, dn.ptr, dzp.ptr, K, 0)
	lay, dense = lc.pixel_layout('frames', T, P), lc.pixel_layout('dense', T, P)

	def evaluate(olay, add=None, astride=0, zoom=None, stride=None):
		dst = out(ctx, olay, 'float32')
		stride = olay.frame_stride if stride is None else stride
		if zoom is None:
			ctx._check(ctx.lib.tp_radial_evaluate(ctx.handle, T, R, C, stride, float(lc.COL_OFFSET), float(geo.xcen), float(geo.ycen), dk.ptr, dc.ptr, dn.ptr, K,
				dzp.ptr, None if add is None else add.ptr, astride, dst.ptr))
		else:
			ctx._check(ctx.lib.tp_radial_evaluate_zoom(ctx.handle, T, R, C, stride, ctypes.byref(spec), ctypes.byref(zoom), dst.ptr))
		ctx.sync()
		return dst.image().reshape(T, R, C)

	radial, radial0 = evaluate(lay), evaluate(dense)
	np.testing.assert_array_equal(radial, radial0)
	np.testing.assert_allclose(radial, want, rtol=2e-7, atol=1e-5)
	# the square component to add: stored per frame (padded stride of its own) and implicit
	dlay = lc.Layout('dense', T, R, C)
	src0 = put(ctx, dlay, f, poison)
	mesh, nm = _mesh(ctx, src0, dlay)
	z = Zoomed(ctx, mesh, nm)
	square = z.image(ctx, dlay)
	alay = lc.pixel_layout('frames', T, P, frame_pad=5)
	d_add, d_add0 = put(ctx, alay, square.reshape(T, 1, P), poison), put(ctx, dense, square.reshape(T, 1, P), poison)
	total = evaluate(lay, add=d_add, astride=alay.frame_stride)
	np.testing.assert_allclose(total, want + square.astype('float64'), rtol=2e-7, atol=1e-5)
	for other in (evaluate(dense, add=d_add0, astride=P), evaluate(lay, zoom=z.spec(C)), evaluate(dense, zoom=z.spec(C))):
		np.testing.assert_array_equal(other, total)
	with pytest.raises(_error(), match='tp_radial_evaluate: add_frame_stride must be 0 or at least'):
		evaluate(lay, add=d_add0, astride=P - 1)
	with pytest.raises(_error(), match='tp_radial_evaluate: bad frame geometry'):
		evaluate(dense, stride=P - 1)
	# ---- the mesh with the radial component taken off: implicit on every layout == stored, and stored against the oracle
	d_radial = ctx.array(radial0)
	stored, stored_nm = _mesh(ctx, src0, dlay, subtract=d_radial, sstride=P)
	m0, n0 = stored.host(), stored_nm.host()
	for k, (ref_mesh, ref_nm) in enumerate(lc.mesh_expected(f, subtract=radial0)):
		np.testing.assert_array_equal(n0[k], ref_nm)
		np.testing.assert_allclose(m0[k], ref_mesh, rtol=1e-9, equal_nan=True)
	d_ex1 = ctx.array(lc.exclude_image(R, C))
	stored_ex, stored_ex_nm = _mesh(ctx, src0, dlay, subtract=d_radial, sstride=P, exclude=d_ex1, estride=0)
	for kind in ('dense',) + lc.LAYOUTS:
		klay = lc.Layout(kind, T, R, C)
		src = put(ctx, klay, f, poison)
		mesh, nm = _mesh(ctx, src, klay, radial=spec)
		np.testing.assert_array_equal(nm.host(), n0, err_msg=kind)
		np.testing.assert_array_equal(mesh.host(), m0, err_msg=kind)
		mesh, nm = _mesh(ctx, src, klay, radial=spec, exclude=d_ex1, estride=0)
		np.testing.assert_array_equal(nm.host(), stored_ex_nm.host(), err_msg=kind)
		np.testing.assert_array_equal(mesh.host(), stored_ex.host(), err_msg=kind)
