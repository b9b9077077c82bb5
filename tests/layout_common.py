# -*- coding: utf-8 -*-
"""
Frame-stack layouts for the tests of the C entries that take ``row_pitch`` / ``frame_stride`` (include/tessphot_hip.h, "the prepare
stage on a frame stack", the stamp cutter, the radial component): the same ``(T, R, C)`` values embedded in a flat buffer as

* ``rows``     ``row_pitch = C + 1`` (odd: rows lose their 16-byte alignment), ``rows13``: ``C + 13``;
* ``frames``   dense rows, ``frame_stride = R * C + 7``;
* ``window``   the window ``[r0:r0 + R, c0:c0 + C]`` of a larger stack ``(T, RR, CC)``: ``row_pitch = CC``, ``frame_stride = RR * CC``,
               the pointer handed over lies ``r0 * CC + c0`` elements inside the allocation (neither ``c0`` nor that offset a multiple of 4);
* ``dense``    the layout the product itself passes.

Every buffer ends in a band of ``TAIL`` elements beyond the last element a correct kernel may address.  Inputs carry poison in every
element outside the image, outputs a guard pattern that must come back untouched.  The case tables of tests/test_gpu_frame_layouts.py
live here too, with the data and the references (oracle, scipy, numpy -- never the library), so that tests/test_layout_common.py can
hold them to the geometry the entries require without a GPU.
"""
import numpy as np

TAIL = 64
LAYOUTS = ('rows', 'rows13', 'frames', 'window')
POISONS = (np.nan, 1e30)
WINDOW_R0, WINDOW_C0 = 3, 5


class Layout(object):
	"""Where pixel ``(k, r, c)`` of a ``(T, R, C)`` stack sits in a flat buffer: ``offset + k * frame_stride + r * row_pitch + c``."""

	def __init__(self, kind, T, R, C, frame_pad=7):
		self.kind, self.T, self.R, self.C = kind, int(T), int(R), int(C)
		T, R, C = self.T, self.R, self.C
		self.offset = 0
		if kind == 'dense':
			self.row_pitch, self.frame_stride = C, R * C
		elif kind == 'rows':
			self.row_pitch = C + 1
			self.frame_stride = R * self.row_pitch
		elif kind == 'rows13':
			self.row_pitch = C + 13
			self.frame_stride = R * self.row_pitch
		elif kind == 'frames':
			self.row_pitch, self.frame_stride = C, R * C + int(frame_pad)
		elif kind == 'window':
			RR, CC = R + WINDOW_R0 + 2, C + WINDOW_C0 + 6
			if (WINDOW_R0 * CC + WINDOW_C0) % 4 == 0:
				CC += 1
			self.row_pitch, self.frame_stride = CC, RR * CC
			self.offset = WINDOW_R0 * CC + WINDOW_C0
			self.outer = (T, RR, CC)
		else:
			raise ValueError(kind)
		# the whole allocation: every frame's full stride (the larger stack of a window), then the band
		self.size = T * self.frame_stride + TAIL
		self.last = self.offset + (T - 1) * self.frame_stride + (R - 1) * self.row_pitch + C - 1   # last element the contract lets a kernel touch
		assert self.last < self.size - TAIL

	def index(self):
		"""int64 ``(T, R, C)``: the flat position of every pixel."""
		k, r, c = np.ogrid[0:self.T, 0:self.R, 0:self.C]
		return self.offset + k * np.int64(self.frame_stride) + r * np.int64(self.row_pitch) + c

	def image_mask(self):
		"""bool ``(size,)``: True where the buffer holds a pixel of the image; everything else is poison (inputs) or guard (outputs)."""
		m = np.zeros(self.size, dtype=bool)
		m[self.index().ravel()] = True
		return m

	def embed(self, array, fill):
		"""The flat buffer with ``array`` in place and ``fill`` in every other element."""
		array = np.asarray(array)
		assert array.shape == (self.T, self.R, self.C), (array.shape, (self.T, self.R, self.C))
		flat = np.full(self.size, fill, dtype=array.dtype)
		flat[self.index().ravel()] = array.ravel()
		return flat

	def extract(self, flat):
		flat = np.asarray(flat)
		assert flat.shape == (self.size,)
		return flat[self.index()]

	def args(self):
		"""``(row_pitch, frame_stride)`` as the C entries take them."""
		return self.row_pitch, self.frame_stride


def pixel_layout(kind, T, n_pixels, frame_pad=7):
	"""The layout of an entry that takes ``n_pixels`` and ``frame_stride`` only (contiguous images): one row per frame."""
	assert kind in ('dense', 'frames')
	return Layout(kind, T, 1, n_pixels, frame_pad=frame_pad)


GUARD32 = np.array([0x7b7b7b7b], dtype='uint32').view('float32')[0]   # a pattern no kernel produces


def guard_of(dtype):
	dtype = np.dtype(dtype)
	return np.frombuffer(b'\x7b' * dtype.itemsize, dtype=dtype)[0]


def guard_buffer(layout, dtype):
	"""An output buffer full of the guard pattern."""
	return np.full(layout.size, guard_of(dtype), dtype=dtype)


def guard_intact(layout, flat):
	"""True if every element outside the image still holds the guard pattern (compared as bytes: the pattern may be a NaN elsewhere)."""
	flat = np.asarray(flat)
	raw = flat.view('uint8').reshape(flat.size, flat.dtype.itemsize)
	return bool(np.all(raw[~layout.image_mask()] == 0x7b))


def dense_guarded(shape, dtype):
	"""A dense output ``shape`` followed by the band: ``(flat buffer full of guard, number of real elements)``."""
	n = int(np.prod(shape, dtype='int64'))
	return np.full(n + TAIL, guard_of(dtype), dtype=dtype), n


def dense_tail_intact(flat, n):
	raw = np.asarray(flat).view('uint8')
	return bool(np.all(raw[n * flat.dtype.itemsize:] == 0x7b))


# ---------------------------------------------------------------------------------------------------------------------------------
# stamp cutter, sum-image crop
# ---------------------------------------------------------------------------------------------------------------------------------
COL_OFFSET = 44
# (T, R, C, H, W, n): the first is a dense batch (frame-tile-major path), the second a sparse one (per-stamp gather); test_gpu_cutout.py's shapes
CUT_CASES = [(70, 60, 130, 15, 15, 300), (33, 200, 300, 21, 11, 4)]


def cut_path(R, C, H, W, n):
	"""Which kernel cut_stamps_launch (csrc/cutout.hip) picks: stamps covering at least an eighth of the frame go tile by tile."""
	return 'tiles' if n * H * W * 8 >= R * C else 'gather'


def cut_frames(T, R, C, seed):
	rng = np.random.default_rng(seed)
	f = rng.normal(0, 1, (T, R, C)).astype('float32')
	f[rng.random((T, R, C)) < 0.02] = np.nan
	return f


def cut_stamps(R, C, H, W, n, seed):
	"""int32 ``(n + 8, 4)`` stamps in CCD coordinates: random ones reaching up to three pixels over every edge, then one sticking out on
	each side and at each corner of the frame."""
	rng = np.random.default_rng(seed)
	r0 = rng.integers(-3, R - H + 4, n)
	c0 = rng.integers(-3, C - W + 4, n)
	edge = [(-2, C // 2), (R - H + 2, C // 2), (R // 2, -2), (R // 2, C - W + 2), (-1, -1), (-1, C - W + 1), (R - H + 1, -1), (R - H + 1, C - W + 1)]
	r0 = np.concatenate((r0, [e[0] for e in edge]))
	c0 = np.concatenate((c0, [e[1] for e in edge])) + COL_OFFSET
	return np.stack((r0, r0 + H, c0, c0 + W), axis=1).astype('int32')


def crop_expected(full, stamp, row_offset, col_offset):
	"""``full[ir1:ir2, ic1:ic2]`` (BasePhotometry.py:1001-1006) with NaN where the stamp leaves the image."""
	R, C = full.shape
	r1, r2, c1, c2 = (int(v) for v in stamp)
	r1, r2, c1, c2 = r1 - row_offset, r2 - row_offset, c1 - col_offset, c2 - col_offset
	out = np.full((r2 - r1, c2 - c1), np.nan)
	ra, rb, ca, cb = max(r1, 0), min(r2, R), max(c1, 0), min(c2, C)
	if ra < rb and ca < cb:
		out[ra - r1:rb - r1, ca - c1:cb - c1] = full[ra:rb, ca:cb]
	return out


# ---------------------------------------------------------------------------------------------------------------------------------
# transpose, smoothing, sum image, block median
# ---------------------------------------------------------------------------------------------------------------------------------
# (n_frames, n_pixels, t_pitch): frames off the 64 block, pixels off the 64 tile, t_pitch equal to n_frames and larger
TRANSPOSE_CASES = [(70, 1003, 70), (70, 1003, 96), (129, 197, 160), (64, 128, 64), (5, 63, 8)]
TIME_CASE = (30, 37, 53)      # (T, R, C) of the smoothing / sum-image case


def time_frames(seed=4):
	T, R, C = TIME_CASE
	rng = np.random.default_rng(seed)
	f = rng.normal(100, 5, (T, R, C)).astype('float32')
	f[rng.random((T, R, C)) < 0.05] = np.nan
	f[:, 3, 4] = np.nan                 # a pixel without any value
	f[7, 5, 6] = np.inf
	quality = np.zeros(T, dtype='int32')
	quality[[2, 11]] = 32               # bad frames: left out of the sum image
	return f, quality


# ---------------------------------------------------------------------------------------------------------------------------------
# median filter
# ---------------------------------------------------------------------------------------------------------------------------------
MEDIAN_LAYOUT_SHAPE = (2, 37, 141)
MEDIAN_LAYOUT_SIZES = (15, 11, 5)
MEDIAN_SIZES = (3, 7, 9, 11, 13, 15)
# widths either side of 32 (a workgroup of the general kernels) and of 128 (a workgroup of the 15 x 15 kernel); one dimension below every window from 9 on
MEDIAN_SHAPES = [(33, 31), (33, 33), (17, 127), (17, 129), (8, 40), (40, 8)]


def median_kernel(size, R, C):
	"""The kernel tp_frames_median_filter launches (csrc/background.hip)."""
	fast = R >= size and C >= size and size >= 8
	if size == 15 and fast:
		return 'tp_median15_quad_kernel'
	return 'tp_median_filter_kernel<32, true>' if fast else 'tp_median_filter_kernel<32, false>'


def median_frames(T, R, C, seed):
	rng = np.random.default_rng(seed)
	img = rng.normal(0, 3, (T, R, C)).astype('float32')
	img[0, R // 2:, :C // 3] = rng.integers(-2, 3, (R - R // 2, C // 3)).astype('float32')   # many equal values
	bad = rng.random((T, R, C)) < 0.02
	img[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype='float32'), int(bad.sum()))
	ref = rng.normal(0, 1, (R, C))
	return img, ref


def median_expected(img, ref, size):
	"""scipy on the same values, as tests/test_gpu_fullframe.py::test_median_filter_15_shared_columns forms it."""
	from scipy.ndimage import median_filter
	x = (img.astype('float64') - ref).astype('float32') if ref is not None else img.copy()
	x[~np.isfinite(x)] = np.inf
	want = median_filter(x, size=size)
	want[~np.isfinite(want)] = np.nan
	return want


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel flags
# ---------------------------------------------------------------------------------------------------------------------------------
def flag_frames():
	"""``(frames (T, R, C), first excluded column per frame)``: frame 2 is zero everywhere (excluded as a whole for TESS data)."""
	T, R, C = 4, 20, 70
	rng = np.random.default_rng(12)
	f = (100 + rng.normal(0, 3, (T, R, C))).astype('float32')
	f[0, 3:9, 10:20] = np.nan
	f[1, 2:5, 60:65] = 2e5
	f[3, 4, 5] = -1.0
	f[3, 6, 7] = 0.0
	f[2] = 0.0
	return f, np.array([C, 50, C, C], dtype='int32')


def flag_expected(f, first):
	from oracle import backgrounds as ob
	T, R, C = f.shape
	zero = np.array([bool(np.all(f[k] == 0)) for k in range(T)])
	manexcl = np.zeros(f.shape, dtype=bool)
	for k in range(T):
		manexcl[k, :, int(first[k]):] = True
		if zero[k]:
			manexcl[k] = True                              # pixel_flags.py:54-56
	masks = np.stack([ob.stamp_mask(f[k], 8e4, manexcl[k]) for k in range(T)])
	flags, _ = ob.prepare_pixel_flags(f, masks, manexcl)
	return flags, zero


# ---------------------------------------------------------------------------------------------------------------------------------
# full-frame background: mesh, zoom
# ---------------------------------------------------------------------------------------------------------------------------------
MESH_CASES = [(2, 300, 421), (2, 150, 131)]     # no multiple of the 64-pixel box


def sky_frames(T, R, C, seed):
	rng = np.random.default_rng(seed)
	yy, xx = np.mgrid[0:R, 0:C]
	sky = 100 + 0.03 * xx + 0.015 * yy + 5 * np.sin(xx / 90.0)
	f = np.empty((T, R, C), dtype='float32')
	for k in range(T):
		img = sky * (1 + 0.02 * np.sin(k)) + rng.normal(0, 3, (R, C))
		for _ in range(40):
			r, c = rng.integers(0, R), rng.integers(0, C)
			img[max(r - 2, 0):r + 3, max(c - 2, 0):c + 3] += rng.uniform(500, 90000)
		f[k] = img
	f[0, 10:20, 30:40] = np.nan
	f[1, 64:128, 0:64] = -5.0            # a cell that is masked whole: filled from its neighbours
	return f


def exclude_image(R, C):
	ex = np.zeros((R, C), dtype='uint8')
	ex[:, C - 37:] = 1
	ex[R // 3:R // 3 + 40, 50:90] = 1
	return ex


def subtract_images(T, R, C):
	"""A smooth float32 image per frame, different from frame to frame (what the radial component looks like)."""
	yy, xx = np.mgrid[0:R, 0:C]
	return np.stack([(3.0 + k) * np.exp((xx + yy) / float(R + C)) for k in range(T)]).astype('float32')


def mesh_expected(f, exclude=None, subtract=None, box=64):
	"""Per frame ``(mesh, nmasked)`` of the oracle: the pixel mask on the raw image, the statistics on float32(img - subtract)."""
	from oracle import backgrounds as ob
	out = []
	for k in range(f.shape[0]):
		ex = None if exclude is None else (exclude if exclude.ndim == 2 else exclude[k]).astype(bool)
		mask = ob.stamp_mask(f[k], 8e4, ex)
		img = f[k] if subtract is None else (f[k].astype('float64') - subtract[k].astype('float64')).astype('float32')
		out.append(ob.mesh_statistics(img, mask, box=box))
	return out


# ---------------------------------------------------------------------------------------------------------------------------------
# radial component
# ---------------------------------------------------------------------------------------------------------------------------------
RADIAL_CASE = (2, 320, 384)      # the corner of camera 1, CCD 1, as tests/test_gpu_fullframe.py::test_radial_pieces


def tess_frames(T, R, C, seed, xcen, ycen):
	rng = np.random.default_rng(seed)
	yy, xx = np.mgrid[0:R, 0:C]
	r = np.hypot(xx + COL_OFFSET - xcen, yy - ycen)
	f = np.empty((T, R, C), dtype='float32')
	for k in range(T):
		glow = (40 + 10 * k) * np.exp((r - 2400) / 250.0)
		img = 120 + 0.02 * xx + glow + rng.normal(0, 4, (R, C))
		for _ in range(60):
			y, x = rng.integers(0, R), rng.integers(0, C)
			img[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] += rng.uniform(500, 90000)
		f[k] = img
	f[0, 5:9, 7:30] = np.nan
	f[-1, 100:164, 200:264] = -3.0
	return f


def radial_mask(f, exclude=None):
	m = ~np.isfinite(f) | (f > 8e4) | (f < 0)
	if exclude is not None:
		m = m | exclude.astype(bool)
	return m


def ring_profile(bin_center):
	"""A known ring profile with three rings missing, per frame a different level."""
	y = np.stack([2.0 + 0.3 * np.sin(bin_center / 100.0), 2.1 + 0.2 * np.cos(bin_center / 80.0)])
	y[0, [3, 4, 17]] = np.nan
	return y


def radial_expected(y, bin_center, zeropoint, R, C, xcen, ycen):
	"""``10**spline(r) - zeropoint`` with scipy on the distance image (backgrounds.py:186-188)."""
	from scipy.interpolate import InterpolatedUnivariateSpline
	yy, xx = np.mgrid[0:R, 0:C]
	r = np.sqrt((xx + COL_OFFSET - xcen)**2 + (yy - ycen)**2)
	good = ~np.isnan(y)
	return 10**InterpolatedUnivariateSpline(bin_center[good], y[good], k=3, ext=3)(r) - zeropoint
