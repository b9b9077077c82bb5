# -*- coding: utf-8 -*-
"""
B*'s pixel mask is settled per REGISTER ROW (background.hip, bkg_frame_sort): a row of the wavefront -- pixels 8 j .. 8 j + 7 of
its eight frames -- without a masked value skips the mask statements by a scalar branch.  The parity tests of
test_gpu_background.py draw NaN at random (a quarter of the rows dirty, anywhere); here the cubes are CLEAN and single values
are planted at the seams of that layout: the lanes and rows of a frame (pixels 0, 7, 8, the last pixel of the last complete
row, the partial row), the frames of a wavefront and the blocks of a series (cadences 0, 7, 8, 31, 32, 39), every value the
mask decides on (either side of the cutoff, both zeros, the infinities, NaN), frames with a masked value in every row, frames
more than half and wholly masked, beside a target left clean.

Asserted, for the 15 x 15 and 11 x 11 instances (also at the other pixel counts they serve: an empty partial row, a full one but
for a pixel) and the 16 x 16 one (the instance that tests every slot): the stamp background
of tp_background_stamp and of tp_background_sumimage bit for bit the oracle's (oracle/backgrounds.py, NaN positions included),
the smoothed series bit for bit tp_smooth_time's, the sum image within 1e-12 of the oracle's chain from the raw cube (float64
sums of the same float32 differences in another order: the bound of test_gpu_raw_chain.py).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CUTOFF = np.float32(8e4)
VALUES = {
	'nan': np.float32(np.nan), 'pinf': np.float32(np.inf), 'ninf': np.float32(-np.inf), 'minus1': np.float32(-1.0),
	'minus0': np.float32(-0.0), 'plus0': np.float32(0.0), 'cutoff': CUTOFF, 'above': np.nextafter(CUTOFF, np.float32(np.inf)),
	'9e4': np.float32(9e4),
}
MASKED = ('nan', 'pinf', 'ninf', 'minus1', 'above', '9e4')      # the others are kept: -0.0 is not < 0, the cutoff itself is not > cutoff
SHAPES = [(2, 40, 15, 15), (2, 40, 11, 11), (2, 12, 16, 16),  # a full block + a block of 8 frames: <28,*>, <15,*>; one short block: <-1,*>
	# the other fill levels of the two tuned instances' partial row (they serve n_pix 224 .. 231 and 120 .. 127): 224 and 120 with no
	# pixel in it, 228 (also the one-pass kernel's frame_stride += 8), 231 and 127 with seven
	(2, 40, 14, 16), (2, 40, 12, 19), (2, 40, 7, 33), (2, 40, 15, 8), (2, 40, 1, 127)]
CUTOFF_SHAPES = SHAPES[:2] + [(2, 40, 14, 16), (2, 40, 15, 8)]   # ... and the sizes at which the <-1> instances run without a partial row


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


_BASE = {}


def _base(shape, nan_fraction=0.0):
	"""The clean cube of a shape (made once, never written to: every case plants into a copy)."""
	key = (shape, nan_fraction)
	if key not in _BASE:
		from photometry_amd import simulate
		nt, T, H, W = shape
		s = simulate.make_scene(nt, T, H, W, seed=700 + H)
		simulate.fill_cubes(s, nan_fraction=nan_fraction, with_raw=True)
		q = s.quality.astype('int32').copy()
		q[T // 2] |= 32
		for a in (s.raw, s.raw_err, q):
			a.setflags(write=False)
		_BASE[key] = (s.raw, s.raw_err, q)
	return _BASE[key]


def _places(shape):
	"""Pixels (row-major index; pixel p sits in register row p // 8 of lane p % 8) and cadences at the seams."""
	nt, T, H, W = shape
	P = H * W
	jfull = P // 8
	partial = list(range(8 * jfull, P)) or [P - 1]          # 16 x 16 has no partial row: its last pixel
	pixels = [p for p in [0, 7, 8, 8 * jfull - 1] + partial if 0 <= p < P]      # stamps of fewer than nine pixels lack some of them
	cadences = [c for c in (0, 7, 8, 31, 32, 39) if c < T] + ([T - 1] if T < 40 else [])
	return P, pixels, cadences


def _check(ctx, raw, err, q, time_smooth=3, flux_cutoff=8e4):
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	from oracle import backgrounds as ob, sumimage as osum
	nt, H, W, T = raw.shape
	ref = np.stack([ob.background_series(raw[i], flux_cutoff) for i in range(nt)])
	cube, dq = DeviceCube.from_host(ctx, raw), ctx.array(q)
	bkg = engine.background_stamp(ctx, cube, flux_cutoff=flux_cutoff)
	np.testing.assert_array_equal(bkg.to_host()[:, :T], ref)                      # bit for bit, NaN positions included
	b_raw, b_smooth, S = engine.background_sumimage(ctx, cube, dq, time_smooth, flux_cutoff=flux_cutoff)
	np.testing.assert_array_equal(b_raw.to_host()[:, :T], ref)
	smooth = b_smooth.to_host()[:, :T]
	np.testing.assert_array_equal(smooth, engine.smooth_time(ctx, bkg, T, time_smooth).to_host()[:, :T])
	osm = ob.smooth_time(ref, time_smooth)
	np.testing.assert_array_equal(smooth, osm)
	got = S.to_host()
	for i in range(nt):
		img, _ = ob.subtract_background(raw[i], err[i], osm[i][None, None, :])
		np.testing.assert_allclose(got[i], osum.sumimage(img, q), rtol=1e-12, atol=0, equal_nan=True)
	return ref


def _plant_seams(raw, shape, value_of):
	"""Target 0: at the seam cadences every seam pixel, in the cadences after them one seam pixel alone; target 1 stays clean.
	``value_of(i)``: the value of the i-th place."""
	P, pixels, cadences = _places(shape)
	T = shape[1]
	X = raw[0].reshape(P, T)
	i = 0
	for c in cadences:
		for p in pixels:
			X[p, c] = value_of(i); i += 1
	singles = [c for c in range(T) if c not in cadences][:len(pixels)] + ([33, 38] if T >= 40 else [])
	for k, c in enumerate(singles):
		X[pixels[k % len(pixels)], c] = value_of(i); i += 1
	return cadences


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[2]}x{s[3]}")
@pytest.mark.parametrize("name", list(VALUES) + ['all'])
def test_planted_values_at_the_seams(ctx, shape, name):
	raw0, err, q = _base(shape)
	raw = raw0.copy()
	vals = list(VALUES.values())
	_plant_seams(raw, shape, (lambda i: vals[i % len(vals)]) if name == 'all' else (lambda i: VALUES[name]))
	assert not np.array_equal(raw[0], raw0[0], equal_nan=True) and np.array_equal(raw[1], raw0[1])
	ref = _check(ctx, raw, err, q)
	assert np.isfinite(ref).all()                                                 # a handful of masked pixels: every frame has its estimate


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[2]}x{s[3]}")
def test_dirty_frames_among_clean_ones(ctx, shape):
	"""A masked value in every register row of a frame, a frame more than half masked, a frame wholly masked -- in the first
	wavefront of the first block and in the last block -- among clean frames; target 1 clean."""
	raw0, err, q = _base(shape)
	raw = raw0.copy()
	nt, T, H, W = shape
	P = H * W
	X = raw[0].reshape(P, T)
	vals = list(VALUES.values())
	bad = [VALUES[k] for k in MASKED]
	groups = [(2, 3, 4), (T - 6, T - 5, T - 4)]
	for c_rows, c_half, c_all in groups:
		for j in range((P + 7) // 8):
			p = 8 * j + (j % 8)
			if p < P:
				X[p, c_rows] = bad[j % len(bad)]                                      # every row dirty, a different lane each
		for p in range(P // 2 + 1):
			X[p, c_half] = bad[p % len(bad)]
		for p in range(P):
			X[p, c_all] = vals[p % len(vals)] if p % len(vals) not in (4, 5, 6) else bad[p % len(bad)]   # no kept value among them
	ref = _check(ctx, raw, err, q)
	for c_rows, c_half, c_all in groups:
		assert np.isfinite(ref[0, c_rows]) and np.isnan(ref[0, c_half]) and np.isnan(ref[0, c_all])
	assert np.isfinite(ref[1]).all() and np.isfinite(np.delete(ref[0], [c for g in groups for c in g[1:]])).all()


def test_random_nan_rows(ctx):
	"""nan_fraction = 0.004: about a quarter of the rows dirty, the clean and the dirty path interleaved at random."""
	raw, err, q = _base(SHAPES[0], nan_fraction=0.004)
	assert np.isnan(raw).any()
	_check(ctx, raw, err, q)


@pytest.mark.parametrize("shape", CUTOFF_SHAPES, ids=lambda s: f"{s[2]}x{s[3]}")
@pytest.mark.parametrize("cutoff", [-1.0, -0.0, float('nan')])
def test_cutoff_without_an_order(ctx, shape, cutoff):
	"""A negative or NaN cutoff masks every pixel (-0.0: all but the zeros): the integer pre-test of a row does not apply and the
	launch must take the exact statements for every value.  All-NaN series, as the oracle gives."""
	raw0, err, q = _base(shape)
	raw = raw0.copy()
	raw[0, 0, 0, 5] = 0.0                         # +0.0 <= -0.0 holds: kept under the -0.0 cutoff, but one pixel of the stamp is no estimate
	ref = _check(ctx, raw, err, q, flux_cutoff=cutoff)
	assert np.isnan(ref).all()
