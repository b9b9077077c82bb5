# -*- coding: utf-8 -*-
"""
The inputs of test_gpu_background_sizes.py, held to what makes its comparison with the oracle mean something -- the oracle alone,
on the sweep's exact cubes (2 targets x 40 cadences = 80 frames per pixel count, planted values included), no device:

* bstar_frames runs for every swept pixel count, 1 included;
* from 64 pixels on at least 5 frames take three clipping passes or more and at least one frame is clipped at both ends;
* from 16 pixels on fewer than a quarter of the frames are without estimate;
* at the pixel counts of the tuned instances with a partial register row (121 .. 127, 225 .. 231) the estimate without that row
  differs in at least half of the frames that have one: what a kernel that dropped or mis-indexed the row would return;
* the exclude_percentile inputs put a finite and a NaN estimate either side of the float32 comparison.

A size that misses a condition gets another seed (test_gpu_background_sizes.SEEDS), never another condition.
"""
import numpy as np
import pytest

import test_gpu_background_sizes as sizes
from test_gpu_background_sizes import SIZES, NT, T


@pytest.fixture(scope='module')
def states():
	"""P -> (estimates (80,), end state of the clipping) of the oracle on the sweep's frames."""
	from oracle import backgrounds as ob
	return {P: ob.bstar_frames(sizes.frames_of(sizes.sweep_inputs(P)), full=True) for P in SIZES}


def test_the_sweep_is_the_one_asked_for():
	assert SIZES[:264] == list(range(1, 265)) and SIZES[264:] == [511, 512, 513, 1023, 1024, 1025]
	assert sorted(P for g in sizes.GROUPS for P in g) == SIZES and max(len(g) for g in sizes.GROUPS) <= 32
	for P in SIZES:
		H, W = sizes.stamp_of(P)
		assert H * W == P and 1 <= H <= W
		raw = sizes.sweep_inputs(P)
		assert raw.shape == (NT, H, W, T) and raw.dtype == np.float32
	assert sizes.stamp_of(224) == (14, 16) and sizes.stamp_of(228) == (12, 19) and sizes.stamp_of(127) == (1, 127)
	want = set(range(1, 10)) | set(range(29, 33)) | set(range(57, 61)) | set(range(120, 128)) | set(range(224, 233)) | set(range(252, 258))
	assert set(sizes.WINDOW_SIZES) == want and len(sizes.WINDOW_SIZES) == len(want)


def test_frame_stride_branch_sizes():
	"""The pixel counts the GPU file's docstring names for the one-pass kernel's `frame_stride += 8` (tp_background_sumimage: the
	staged frame's stride is a multiple of 32 words), from the host statements restated."""
	def stride(n_pix):
		last = (n_pix - 1) | 3
		return ((last + ((last >> 5) << 2) + 1) + 3) & ~3
	bumped = [P for P in range(1, 257) if stride(P) % 32 == 0]
	assert bumped == [28 * q + 29 + i for q in range(8) for i in range(4)]
	assert set(bumped) <= set(SIZES) and {29, 30, 31, 32, 57, 58, 59, 60, 225, 226, 227, 228} <= set(sizes.WINDOW_SIZES)


def test_planted_values_reach_the_seams():
	"""Target 0 carries every value of VALUES at the seam pixels of each size; target 1 is the generator's own."""
	from test_gpu_background_rows import VALUES, _places
	for P in SIZES:
		H, W = sizes.stamp_of(P)
		_, pixels, cadences = _places((NT, T, H, W))
		assert cadences == [0, 7, 8, 31, 32, 39]
		want = {0, 7, 8, 8 * (P // 8) - 1, P - 1} | set(range(8 * (P // 8), P))
		assert set(pixels) == {p for p in want if 0 <= p < P}
		X = sizes.sweep_inputs(P)[0].reshape(P, T)
		planted = X[sorted(set(pixels))].view('uint32')
		if len(set(pixels)) * len(cadences) >= 2 * len(VALUES):
			for v in VALUES.values():
				assert (planted == np.float32(v).view('uint32')).any(), (P, v)


def test_every_size_has_its_estimates(states):
	for P in SIZES:
		est, st = states[P]
		assert est.shape == (NT * T,) and est.dtype == np.float32
		assert np.array_equal(np.isfinite(est), st['usable']), P
		if P >= 16:
			assert np.isnan(est).sum() < NT * T / 4, (P, int(np.isnan(est).sum()))


def test_the_clipping_is_exercised(states):
	for P in SIZES:
		if P >= 64:
			_, st = states[P]
			deep = int((st['usable'] & (st['passes'] >= 3)).sum())
			both = int((st['usable'] & (st['lo'] > 0) & (st['n'] - st['hi'] > 0)).sum())
			assert deep >= 5 and both >= 1, (P, deep, both)


@pytest.mark.parametrize("P", list(range(121, 128)) + list(range(225, 232)))
def test_the_tail_row_matters(states, P):
	from oracle import backgrounds as ob
	est, _ = states[P]
	X = sizes.frames_of(sizes.sweep_inputs(P))
	cut = ob.bstar_frames(X[:, :8 * (P // 8)])
	have = np.isfinite(est)
	differ = have & ~(est == cut)                     # a NaN without the row differs too
	assert differ.sum() * 2 >= have.sum(), (P, int(differ.sum()), int(have.sum()))


@pytest.mark.parametrize("P", sizes.EXCLUDE_SIZES)
def test_exclude_percentile_inputs(P):
	from test_gpu_background_rows import CUTOFF
	for percentile in sizes.PERCENTILES:
		raw = sizes.exclude_inputs(P, percentile)
		X = sizes.frames_of(raw)
		with np.errstate(invalid='ignore'):
			nmasked = (~((X >= 0) & (X <= CUTOFF))).sum(axis=1).reshape(NT, T)
		k0 = int(np.floor(np.float32(percentile / 100.0) * np.float32(P)))
		for target, cadences in sizes.EXCLUDE_AT:
			assert list(nmasked[target, list(cadences)]) == [min(max(k0 + d, 0), P) for d in (-1, 0, 1)]
			assert nmasked[target].sum() == nmasked[target, list(cadences)].sum()          # the other frames are clean
			x = X[target * T + cadences[1]]
			with np.errstate(invalid='ignore'):
				rows = np.flatnonzero(~((x >= 0) & (x <= CUTOFF))) // 8
			assert len(set(rows)) >= min(k0, P // 8)                                       # spread over the register rows
		sizes.check_exclude_reference(sizes.exclude_reference(raw, percentile), percentile)
