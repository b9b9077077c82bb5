# -*- coding: utf-8 -*-
"""
B* (stamp background) at EVERY pixel count: tp_background_stamp and tp_background_sumimage against the definition
(oracle/backgrounds.py::bstar_frames) for every n_pix in 1 .. 264 and at 511, 512, 513, 1023, 1024, 1025.

Only n_pix = H W enters the kernels.  Which kernel a pixel count reaches, read from photometry_amd/csrc/background.hip (default
flux_cutoff, for which row_pretest_ok, :1056, holds; jfull = n_pix / 8):

* tp_background_stamp (:1073-1098): n_pix <= 256 -> tp_bkg_stamp_kernel<8, JFULL>, by :1082-1085
    <8,28>  jfull == 28: n_pix 224 .. 231         (8 of the sweep's sizes; 0 .. 7 pixels in register row 28)
    <8,15>  jfull == 15: n_pix 120 .. 127         (8 sizes; 0 .. 7 pixels in register row 15)
    <8,-1>  every other n_pix in 1 .. 256         (240 sizes)
  n_pix > 256 -> tp_bkg_stamp_generic_kernel with np2 = the next power of two (:1087-1097): 257 .. 264 (np2 = 512), 511 and 512
  (512), 513, 1023 and 1024 (1024), 1025 (2048): 14 sizes.
* tp_background_sumimage: the one-pass kernel tp_bkg_stamp_sum_kernel<JFULL, W> for n_pix <= 256 and time_smooth <= 17 (:1125),
  JFULL = 28 / 15 / -1 at the same pixel counts (:1141-1150), W = 1, 4 or -1 (run-time window) for time_smooth 3, 9 and the rest
  (:1147); n_pix > 256 goes through tp_background_stamp + tp_smooth_time + tp_sumimage (:1129-1133).
* frame_stride of the one-pass kernel (:1120-1122): with k = (n_pix - 1) / 4 and q = k / 8 it is 4 (k + 1 + q) words, a multiple of 32
  -- the `+= 8` branch -- for n_pix in 28 q + 29 .. 28 q + 32, q = 0 .. 7: 29..32, 57..60, 85..88, 113..116, 141..144, 169..172,
  197..200, 225..228 (restated and checked in test_background_sizes_host.py).

The stamp of a pixel count is its most nearly square factorisation, (1, P) for a prime; the cube descriptor takes every shape
(common.h, tp_desc_ok: height, width > 0).  Frames: _hard_frames of test_gpu_background.py, 2 targets x 40 cadences (a full block of
32 cadences + a block of 8), seed 5000 + P; on target 0 every value of test_gpu_background_rows.VALUES in turn at the seams of the
register layout for that P (_plant_seams of that module).  test_background_sizes_host.py holds these very inputs to what makes
the comparison mean something (deep clips, both ends, few frames without estimate, a tail row that moves the estimate).

Asserted per size: both unsmoothed series bit for bit bstar_frames (NaN positions included), the smoothed series bit for bit
oracle smooth_time, the sum image within 1e-12 of the oracle's chain from the raw cube (subtract_background + sumimage), NaN
positions equal.  time_smooth = 3 everywhere; 1, 9 and 17 as well at the sizes of the tuned instances and next to them, the first
two `+= 8` groups, one register row, and either side of 256.

exclude_percentile acts in one float32 comparison ((float)nmasked > fraction * (float)n_pix, :294 and :960): clean frames with
floor(fraction n_pix) - 1, + 0, + 1 masked pixels, the fraction and the product in float32 as the oracle takes them.
"""
import numpy as np
import pytest

from test_gpu_background import _hard_frames
from test_gpu_background_rows import VALUES, MASKED, _plant_seams

pytestmark = pytest.mark.gpu

NT, T = 2, 40
SIZES = list(range(1, 265)) + [511, 512, 513, 1023, 1024, 1025]
GROUPS = [SIZES[i:i + 32] for i in range(0, len(SIZES), 32)]
WINDOW_SIZES = list(range(1, 10)) + list(range(29, 33)) + list(range(57, 61)) + list(range(120, 128)) + list(range(224, 233)) + list(range(252, 258))
SEEDS = {}                                    # P -> seed where 5000 + P misses a condition of test_background_sizes_host.py (none does)
EXCLUDE_SIZES = (225, 121, 224, 30, 420)
PERCENTILES = (0.0, 10.0, 33.3, 50.0, 66.7, 100.0)
EXCLUDE_AT = ((0, (7, 8, 9)), (1, (31, 32, 33)))      # (target, the cadences with floor - 1, floor, floor + 1 masked pixels)


def stamp_of(P):
	"""(H, W) with H W = P, H the largest divisor <= sqrt(P)."""
	H = max(h for h in range(1, int(P**0.5) + 1) if P % h == 0)
	return H, P // H


def frames_of(raw):
	"""(Nt, H, W, T) cube -> (Nt T, P) frames in row-major stamp order, as bstar_frames takes them."""
	nt, H, W, nc = raw.shape
	return np.ascontiguousarray(np.moveaxis(raw, 3, 1).reshape(nt * nc, H * W))


def quality():
	q = np.zeros(T, dtype='int32')
	q[T // 2] |= 32
	q[T - 1] |= 4
	return q


_INPUTS = {}


def sweep_inputs(P):
	"""The sweep's raw cube (2, H, W, 40) of a pixel count (made once, read-only)."""
	if P not in _INPUTS:
		H, W = stamp_of(P)
		rng = np.random.default_rng(SEEDS.get(P, 5000 + P))
		X = _hard_frames(rng, NT * T, P)
		raw = np.ascontiguousarray(np.moveaxis(X.reshape(NT, T, H, W), 1, 3))
		vals = list(VALUES.values())
		_plant_seams(raw, (NT, T, H, W), lambda i: vals[i % len(vals)])
		raw.setflags(write=False)
		_INPUTS[P] = raw
	return _INPUTS[P]


_ORACLE = {}


def _oracle(P, time_smooth):
	"""(unsmoothed series, smoothed series, sum images) of the oracle for a size and a window (made once, read-only)."""
	from oracle import backgrounds as ob, sumimage as osum
	raw = sweep_inputs(P)
	if P not in _ORACLE:
		ref = ob.bstar_frames(frames_of(raw)).reshape(NT, T)
		ref.setflags(write=False)
		_ORACLE[P] = {'ref': ref}
	o = _ORACLE[P]
	if time_smooth not in o:
		sm = ob.smooth_time(o['ref'], time_smooth)
		err, q = np.ones(raw.shape[1:], dtype='float32'), quality()
		S = np.stack([osum.sumimage(ob.subtract_background(raw[i], err, sm[i][None, None, :])[0], q) for i in range(NT)])
		for a in (sm, S):
			a.setflags(write=False)
		o[time_smooth] = (sm, S)
	return (o['ref'],) + o[time_smooth]


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _check_sizes(ctx, sizes, windows):
	"""Every size is run (a size that misses is named with what it missed, the others still run)."""
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	dq = ctx.array(quality())
	missed = []
	for P in sizes:
		cube = DeviceCube.from_host(ctx, sweep_inputs(P))
		bkg = engine.background_stamp(ctx, cube).to_host()[:, :T]
		for ts in windows:
			ref, sm, S = _oracle(P, ts)
			b_raw, b_smooth, got = engine.background_sumimage(ctx, cube, dq, ts)
			try:
				np.testing.assert_array_equal(bkg, ref, err_msg='tp_background_stamp')             # bit for bit, NaN positions included
				np.testing.assert_array_equal(b_raw.to_host()[:, :T], ref, err_msg='tp_background_sumimage, unsmoothed')
				np.testing.assert_array_equal(b_smooth.to_host()[:, :T], sm, err_msg='tp_background_sumimage, smoothed')
				np.testing.assert_allclose(got.to_host(), S, rtol=1e-12, atol=0, equal_nan=True, err_msg='sum image')
			except AssertionError as e:
				missed.append(f"n_pix = {P} {stamp_of(P)}, time_smooth = {ts}: {e}")
		cube.free()
	assert not missed, "\n".join(missed)


@pytest.mark.parametrize("sizes", GROUPS, ids=lambda g: f"{g[0]}-{g[-1]}")
def test_every_pixel_count(ctx, sizes):
	_check_sizes(ctx, sizes, (3,))


@pytest.mark.parametrize("time_smooth", [1, 9, 17])
def test_other_windows_at_the_seams_of_the_instances(ctx, time_smooth):
	"""W = -1 (time_smooth 1: no window; 17: the run-time window) and W = 4 of the one-pass kernel at the sizes of the two tuned
	instances and either side of them, the first `frame_stride += 8` groups, a single register row, and across 256."""
	_check_sizes(ctx, WINDOW_SIZES, (time_smooth,))


# ---- exclude_percentile

_CLEAN = {}


def exclude_inputs(P, percentile):
	"""Clean frames; at EXCLUDE_AT's cadences floor(frac P) + d masked pixels, d = -1, 0, 1 (held to 0 .. P), taken lane by lane: the
	first of them sit in lane 0 (target 1: lane 7) of every register row in turn."""
	H, W = stamp_of(P)
	if P not in _CLEAN:
		X = np.random.default_rng(7000 + P).normal(100.0, 3.0, (NT * T, P)).astype('float32')
		_CLEAN[P] = np.ascontiguousarray(np.moveaxis(X.reshape(NT, T, H, W), 1, 3))
		_CLEAN[P].setflags(write=False)
	raw = _CLEAN[P].copy()
	frac = np.float32(percentile / 100.0)                 # as bstar_frames takes it
	k0 = int(np.floor(frac * np.float32(P)))
	bad = [VALUES[k] for k in MASKED]
	orders = ([p for g in range(8) for p in range(g, P, 8)], [p for g in range(7, -1, -1) for p in range(g, P, 8)])
	for (target, cadences), order in zip(EXCLUDE_AT, orders):
		Xt = raw[target].reshape(P, T)
		for d, c in zip((-1, 0, 1), cadences):
			for m, p in enumerate(order[:min(max(k0 + d, 0), P)]):
				Xt[p, c] = bad[m % len(bad)]
	return raw


def exclude_reference(raw, percentile):
	from oracle import backgrounds as ob
	return ob.bstar_frames(frames_of(raw), exclude_percentile=percentile).reshape(NT, T)


def check_exclude_reference(ref, percentile):
	"""The oracle's estimates are what the inputs were built for: either side of the comparison among the three frames."""
	for target, cadences in EXCLUDE_AT:
		three = ref[target, list(cadences)]
		if percentile != 100.0:
			assert np.isfinite(three[:2]).all() and np.isnan(three[2]), (percentile, target, three)
		else:
			assert np.isfinite(three[0]) and np.isnan(three[1:]).all(), (percentile, target, three)    # no pixel left: n > 0 fails
		assert np.isfinite(np.delete(ref[target], cadences)).all()


@pytest.mark.parametrize("P", EXCLUDE_SIZES)
def test_exclude_percentile(ctx, P):
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	dq = ctx.array(quality())
	for percentile in PERCENTILES:
		raw = exclude_inputs(P, percentile)
		ref = exclude_reference(raw, percentile)
		check_exclude_reference(ref, percentile)
		cube = DeviceCube.from_host(ctx, raw)
		bkg = engine.background_stamp(ctx, cube, exclude_percentile=percentile).to_host()[:, :T]
		np.testing.assert_array_equal(bkg, ref, err_msg=f'tp_background_stamp, n_pix = {P}, exclude_percentile = {percentile}')
		b_raw, _, _ = engine.background_sumimage(ctx, cube, dq, 3, exclude_percentile=percentile)
		np.testing.assert_array_equal(b_raw.to_host()[:, :T], ref, err_msg=f'tp_background_sumimage, n_pix = {P}, exclude_percentile = {percentile}')
		cube.free()
