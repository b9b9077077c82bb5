# -*- coding: utf-8 -*-
"""
B*'s sigma clipping reads the sorted frame by rank (background.hip, bkg_frame_clip): the two middle ranks, the lowest kept rank,
and from both ends of the kept range eight ranks per step.  The kept range is carried as LDS byte addresses and the ranks are
staged linearly; the layout before put four pad words after every 32 ranks.  The frames here are built for that addressing:

* kept counts n, by NaN-masking, around the multiples of 32 -- 127 .. 129, 159 .. 161, 191 .. 193, 223 .. 225 for 15 x 15, the
  analogous counts for 11 x 11 (63 .. 65, 95 .. 97, 119 .. 121) and 16 x 16 (128, 129, ..., 255, 256): the middle ranks sit on,
  below and above a multiple of 32, for odd and even counts;
* n = 1, 2, 3 of a 3 x 3 stamp, and n = 1, 2, 3 of a 15 x 15 one.  More than half of such a stamp is masked, and the default
  exclude_percentile of 50 gives no estimate: these two cubes are run with exclude_percentile = 100, under which every frame
  with a kept value has its estimate;
* top clips of c bright outliers, c = 0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40.  One pass cannot take them all for the larger c:
  a value is clipped when its distance d from the median exceeds 3 sd, and c equal outliers among m values have
  sd^2 >= (c / m)(1 - c / m) d^2, so c / m < 0.1273 -- 28 of 225, 15 of 121, 32 of 256.  The first 24 (12; 32) outliers are
  therefore far out (1e4 above the sky) and go in the first pass, the others 400 above the sky and go in the second: the walk
  of a pass takes 0 .. 24 (32) ranks, one to four (at 16 x 16: five) steps (11 x 11: c up to 17 only, two steps), and stops
  on, before and after a multiple of 8; the range's upper end comes to lie on, before and after a multiple of 32 (c = 31, 32, 33 of 225: hi = 194, 193, 192).  Six steps in
  one pass would need 40 ranks clipped at once, which the rule does not allow at these sizes;
* bottom clips: b = 1, 8, 9 low outliers together with 9, 1, 9 bright ones, as far below the sky as those are above, so that
  both go in the same pass (together fewer than a ninth of the values) -- the two-sided walk, either side ending before the
  other (the clamp at both ends);
* a ladder: two values at each of five distances (ratio 5) on either side; every one of the five passes moves lo and hi by two;
* two kept values: no clipping ends there (a pass clips fewer than 2 / 9 of its values: the clipped ones have
  (x - med)^2 > 9 sd^2 and all m values together m sd^2 + m (mean - med)^2 <= 2 m sd^2), so it is the masked-down frames
  with n = 2 above that end with two -- the middle ranks are then the whole range;
* the special frames lie on target 0 from cadences 0, 7, 8, 31, 32, 39 on (first and last lanes of a wavefront, of the full block,
  and the block of eight), target 1 is plain sky.

Asserted on the device, for tp_background_stamp and tp_background_sumimage with time_smooth 3 and 9: both unsmoothed series bit
for bit oracle.backgrounds.bstar_frames, the smoothed series bit for bit smooth_time, the sum image within 1e-12 of the oracle's
chain (subtract_background + sumimage), as test_gpu_background_sizes.py asserts it.

test_inputs_reach_the_cases (no device) holds the inputs to what they were built for, from the oracle alone: kept counts, the
clipped counts at both ends, the number of passes from bstar_frames(..., full=True), and the counts pass by pass from the
definition restated (`_trace`), whose end state must be the oracle's.
"""
import numpy as np
import pytest

NT, T = 2, 40
SEAM_CADENCES = (0, 7, 8, 31, 32, 39)
ORDER = list(SEAM_CADENCES) + [c for c in range(T) if c not in SEAM_CADENCES]   # the special frames' cadences, in turn
WINDOWS = (3, 9)
TOP_CLIPS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40)
BOTTOM_CLIPS = ((1, 9), (8, 1), (9, 9))                    # (low outliers, bright outliers)
# name -> (H, W, exclude_percentile, kept counts, outliers of the first pass at most)
CUBES = {
	'15x15': (15, 15, 50.0, (127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225), 24),
	'11x11': (11, 11, 50.0, (63, 64, 65, 95, 96, 97, 119, 120, 121), 12),
	'16x16': (16, 16, 50.0, (128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 255, 256), 32),
	'3x3': (3, 3, 100.0, (1, 2, 3, 1, 2, 3), 0),
	'15x15-few': (15, 15, 100.0, (1, 2, 3, 1, 2, 3), 0),
}


def _frames(name):
	"""[(frame (P,) float32, what it was built for)] of a cube: ``n`` kept values, ``passes`` = [(clipped at the top, at the bottom)]
	pass by pass."""
	H, W, percentile, counts, first = CUBES[name]
	P = H * W
	rng = np.random.default_rng(9100 + P + int(percentile))
	out = []
	for n in counts:
		x = rng.normal(100.0, 3.0, P).astype('float32')
		x[rng.permutation(P)[:P - n]] = np.nan
		out.append((x, {'n': n, 'passes': None}))           # whatever the sky's own tails give
	if first == 0:
		return P, percentile, out
	for c in TOP_CLIPS:
		if c > 2 * first:
			continue                                        # 11 x 11: two passes take 12 + 12 at the most
		x = rng.uniform(98.0, 102.0, P).astype('float32')       # a sky without tails: nothing of it is ever clipped
		at = rng.permutation(P)[:c]
		for i, p in enumerate(at):
			x[p] = (1e4 if i < first else 400.0) + i
		passes = [(min(c, first), 0)] + ([(c - first, 0)] if c > first else [])
		out.append((x, {'n': P, 'passes': [p for p in passes if p != (0, 0)]}))
	for b, c in BOTTOM_CLIPS:
		if 10 * (b + c) >= P:
			continue                                        # 11 x 11: 18 of 121 do not go in one pass (fewer than a ninth do)
		x = rng.uniform(998.0, 1002.0, P).astype('float32')
		at = rng.permutation(P)[:b + c]
		for i, p in enumerate(at[:c]):
			x[p] = 1900.0 + i
		for i, p in enumerate(at[c:]):
			x[p] = 100.0 - i
		out.append((x, {'n': P, 'passes': [(c, b)]}))
	x = rng.uniform(4e4 - 1, 4e4 + 1, P).astype('float32')
	at = rng.permutation(P)[:20]
	for k in range(5):
		d = 30.0 * 5.0**k
		x[at[4 * k]], x[at[4 * k + 1]], x[at[4 * k + 2]], x[at[4 * k + 3]] = 4e4 + d, 4e4 + d + 1, 4e4 - d, 4e4 - d - 1
	out.append((x, {'n': P, 'passes': [(2, 2)] * 5}))
	return P, percentile, out


_INPUTS = {}


def inputs(name):
	"""(raw cube (2, H, W, 40), exclude_percentile, {cadence of target 0: what its frame was built for}) -- made once, read-only."""
	if name not in _INPUTS:
		H, W = CUBES[name][:2]
		P, percentile, special = _frames(name)
		assert len(SEAM_CADENCES) <= len(special) <= T
		X = np.random.default_rng(9200 + P).normal(100.0, 3.0, (NT, T, P)).astype('float32')
		built = {}
		for (x, what), c in zip(special, ORDER):
			X[0, c] = x
			built[c] = what
		raw = np.ascontiguousarray(np.moveaxis(X.reshape(NT, T, H, W), 1, 3))
		raw.setflags(write=False)
		_INPUTS[name] = (raw, percentile, built)
	return _INPUTS[name]


def frames_of(raw):
	nt, H, W, nc = raw.shape
	return np.ascontiguousarray(np.moveaxis(raw, 3, 1).reshape(nt * nc, H * W))


def quality():
	q = np.zeros(T, dtype='int32')
	q[T // 2] |= 32
	return q


_ORACLE = {}


def oracle(name):
	"""{'ref': unsmoothed series, 'state': the clipping's end state, time_smooth: (smoothed series, sum images)} -- made once."""
	if name not in _ORACLE:
		from oracle import backgrounds as ob, sumimage as osum
		raw, percentile, _ = inputs(name)
		est, state = ob.bstar_frames(frames_of(raw), exclude_percentile=percentile, full=True)
		o = {'ref': est.reshape(NT, T), 'state': {k: v.reshape(NT, T) for k, v in state.items()}}
		err, q = np.ones(raw.shape[1:], dtype='float32'), quality()
		for ts in WINDOWS:
			sm = ob.smooth_time(o['ref'], ts)
			S = np.stack([osum.sumimage(ob.subtract_background(raw[i], err, sm[i][None, None, :])[0], q) for i in range(NT)])
			o[ts] = (sm, S)
		for a in [o['ref']] + [a for ts in WINDOWS for a in o[ts]]:
			a.setflags(write=False)
		_ORACLE[name] = o
	return _ORACLE[name]


def _trace(x, flux_cutoff=8e4):
	"""The clipping of one frame from its definition (oracle/backgrounds.py, module header): [(clipped at the top, at the bottom)] of
	every pass that clips, and the end state (lo, hi)."""
	with np.errstate(invalid='ignore'):
		k = np.sort(x[(x >= 0) & (x <= np.float32(flux_cutoff))].astype('float64'))
	lo, hi, passes = 0, len(k), []
	for _ in range(5):
		kept = k[lo:hi]
		m = float(hi - lo)
		s1, s2 = kept.sum(), (kept * kept).sum()
		q9 = max(9.0 * (m * s2 - s1 * s1), 0.0)
		d = (kept - np.median(kept)) * m
		na, nb = int(((d * d > q9) & (d > 0)).sum()), int(((d * d > q9) & (d < 0)).sum())
		if na == 0 and nb == 0:
			break
		passes.append((na, nb))
		lo, hi = lo + nb, hi - na
	return passes, lo, hi


@pytest.mark.parametrize("name", list(CUBES))
def test_inputs_reach_the_cases(name):
	raw, percentile, built = inputs(name)
	o = oracle(name)
	st = o['state']
	X = frames_of(raw)
	assert set(SEAM_CADENCES) <= set(built)
	counts = CUBES[name][3]
	assert sorted(w['n'] for w in built.values() if w['passes'] is None) == sorted(counts)
	steps, moved_both = set(), 0
	for c, what in built.items():
		assert st['usable'][0, c] and np.isfinite(o['ref'][0, c]), (name, c)           # below the exclusion: an estimate exists
		assert st['n'][0, c] == what['n'], (name, c)
		passes, lo, hi = _trace(X[c])
		assert (lo, hi) == (st['lo'][0, c], st['hi'][0, c]) and len(passes) == st['passes'][0, c], (name, c, passes)
		if what['passes'] is not None:
			assert passes == what['passes'], (name, c, passes, what)
			assert st['lo'][0, c] == sum(p[1] for p in passes) and what['n'] - st['hi'][0, c] == sum(p[0] for p in passes)
		steps |= {p[0] // 8 + 1 for p in passes if p[1] == 0}
		moved_both += (len(passes) == 5 and all(p[0] > 0 and p[1] > 0 for p in passes))
	# the middle ranks of the kept counts: on, below and above a multiple of 32, with odd and even counts
	mid = [(n >> 1) % 32 for n in counts]
	if name in ('15x15', '11x11', '16x16'):
		assert {0, 31} <= set(mid) and {n & 1 for n in counts} == {0, 1}
		assert steps >= ({1, 2, 3, 4, 5} if name == '16x16' else {1, 2, 3, 4} if name == '15x15' else {1, 2})
		assert moved_both == 1
		his = {int(st['hi'][0, c]) for c in built}
		if name == '15x15':
			assert {192, 193, 194} <= his                     # the range's upper end on, above a multiple of 32 (c = 33, 32, 31)
			two_sided = [p for w in built.values() if w['passes'] for p in w['passes'] if p[1] > 0]
			assert {(9, 1), (1, 8), (9, 9)} <= set(two_sided)
	else:
		assert sorted(int(st['hi'][0, c] - st['lo'][0, c]) for c in built) == [1, 1, 2, 2, 3, 3]   # two kept values among them
	assert np.isfinite(o['ref'][1]).all()                     # the plain target


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CUBES))
def test_clip_ranks_against_the_oracle(ctx, name):
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	raw, percentile, _ = inputs(name)
	o = oracle(name)
	cube, dq = DeviceCube.from_host(ctx, raw), ctx.array(quality())
	bkg = engine.background_stamp(ctx, cube, exclude_percentile=percentile).to_host()[:, :T]
	np.testing.assert_array_equal(bkg, o['ref'], err_msg='tp_background_stamp')               # bit for bit, NaN positions included
	for ts in WINDOWS:
		sm, S = o[ts]
		b_raw, b_smooth, got = engine.background_sumimage(ctx, cube, dq, ts, exclude_percentile=percentile)
		np.testing.assert_array_equal(b_raw.to_host()[:, :T], o['ref'], err_msg=f'tp_background_sumimage, unsmoothed, time_smooth = {ts}')
		np.testing.assert_array_equal(b_smooth.to_host()[:, :T], sm, err_msg=f'tp_background_sumimage, smoothed, time_smooth = {ts}')
		np.testing.assert_allclose(got.to_host(), S, rtol=1e-12, atol=0, equal_nan=True, err_msg=f'sum image, time_smooth = {ts}')
	cube.free()
