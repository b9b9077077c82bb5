# -*- coding: utf-8 -*-
"""
CPU check of the frames engine's device-free rules (photometry_amd/csrc/frames_rules.h): the header compiled for the host with
AddressSanitizer and UBSan into the driver tests/hostsim/frames_rules_host.cpp, and held -- integers and float32 / float64 values bit
for bit -- to the Python it restates: pipeline._CatalogIndex / _catalogs_of_stamps, comm.packed_block_layout and the table
FramesJob.collect walks, the metadata fields of pipeline.ApertureBatch, stamps.py and plugins.mask_outcome, np.add.reduce.
"""
import itertools
import os
import subprocess
import numpy as np
import pytest
import conftest
from photometry_amd import comm, pipeline, plugins, stamps

SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'frames_rules_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'frames_rules_host')


@pytest.fixture(scope='module')
def driver():
	os.makedirs(OUT_DIR, exist_ok=True)
	subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall',
		'-I' + os.path.join(conftest.ROOT, 'photometry_amd', 'csrc'), '-o', OUT, SRC], check=True)

	def run(text):
		r = subprocess.run([OUT], input=text, capture_output=True, text=True, timeout=120)
		assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
		assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
		assert r.stderr == '', r.stderr
		return r.stdout.splitlines()
	return run


def _hex64(values):
	return ' '.join('%016x' % v for v in np.asarray(values, dtype='float64').ravel().view('uint64'))


def _hex32(values):
	return ' '.join('%08x' % v for v in np.asarray(values, dtype='float32').ravel().view('uint32'))


def _ints(line):
	return [int(v) for v in line.split()]


def _bits(line):
	return [int(v, 16) for v in line.split()]


# ---- catalogue selection ------------------------------------------------------------------------------------------------------
def _catalog(row, col, seed=0):
	rng = np.random.default_rng(seed)
	n = len(row)
	return {'starid': rng.permutation(n).astype('int64') + 100, 'tmag': rng.uniform(4, 16, n).astype('float32'),
		'row': np.asarray(row, dtype='float64'), 'column': np.asarray(col, dtype='float64')}


def _catalog_text(cat):
	lines = ['catalog %d' % len(cat['starid'])]
	for i in range(len(cat['starid'])):
		lines.append('%d %s %s %s' % (cat['starid'][i], _hex32(cat['tmag'][i]), _hex64(cat['row'][i]), _hex64(cat['column'][i])))
	return lines


def _select_text(st, runs):
	return ['select %d %d' % (len(st), runs)] + [' '.join(str(int(v)) for v in s) for s in st]


def _check_selection(out, cat, st):
	offsets, arrays = pipeline._catalogs_of_stamps(pipeline._CatalogIndex(cat), st)
	assert len(out) == 7
	assert _ints(out[0]) == [int(v) for v in offsets]
	assert _ints(out[1]) == [int(v) for v in arrays['starid']]
	for line, name in zip(out[2:], ('tmag', 'row', 'column', 'row_stamp', 'column_stamp')):
		assert arrays[name].dtype == np.float32
		assert _bits(line) == [int(v) for v in arrays[name].view('uint32')], name


def _random_catalog():
	rng = np.random.default_rng(11)
	row, col = rng.uniform(-3, 140, 400), rng.uniform(40, 260, 400)
	row[rng.choice(400, 9, replace=False)] = np.nan
	col[rng.choice(400, 9, replace=False)] = np.nan
	row[5] = np.inf
	return _catalog(row, col, seed=2), rng


def _random_stamps(rng, n):
	r1, c1 = rng.integers(-30, 150, n), rng.integers(10, 280, n)
	return np.stack((r1, r1 + rng.integers(1, 40, n), c1, c1 + rng.integers(1, 40, n)), axis=1)


#: (r1, r2, c1, c2) = (20, 35, 60, 75): row >= 14.5, row < 39.5, column >= 54.5, column < 79.5
_BOUND_STAMP = (20, 35, 60, 75)


def _catalog_cases():
	cases = {}
	cases['empty'] = (_catalog([], []), [_BOUND_STAMP, (0, 1, 0, 1)])
	cases['one_star'] = (_catalog([25.25], [66.5]), [_BOUND_STAMP, (25, 26, 66, 67), (31, 46, 60, 75), (100, 115, 60, 75)])
	cat, rng = _random_catalog()
	cases['random_with_nan'] = (cat, _random_stamps(rng, 60))
	r1, r2, c1, c2 = _BOUND_STAMP
	eps = 2.0**-40
	rows = [r1 - 5.5, r1 - 5.5 - eps, r2 + 4.5, r2 + 4.5 - eps, 30.0, 30.0, 30.0, 30.0, r1 - 5.5, r2 + 4.5]
	cols = [70.0, 70.0, 70.0, 70.0, c1 - 5.5, c1 - 5.5 - eps, c2 + 4.5, c2 + 4.5 - eps, c1 - 5.5, c2 + 4.5 - eps]
	cases['on_the_bounds'] = (_catalog(rows, cols), [_BOUND_STAMP, (r1 + 1, r2 - 1, c1 + 1, c2 - 1), (r1 - 1, r2 + 1, c1 - 1, c2 + 1)])
	cat, rng = _random_catalog()
	cases['outside_each_side'] = (cat, [(-80, -60, 100, 120), (400, 420, 100, 120), (50, 70, -90, -70), (50, 70, 600, 640),
		(-80, -60, -90, -70), (400, 420, 600, 640)])
	cases['covers_it_all'] = (cat, [(-100, 1000, -100, 1000), (-3, 140, 40, 260)])
	return cases


@pytest.mark.parametrize('case', sorted(_catalog_cases()))
def test_catalog_selection_equals_python(driver, case):
	cat, st = _catalog_cases()[case]
	st = np.asarray(st, dtype='int64')
	out = driver('\n'.join(_catalog_text(cat) + _select_text(st, 1)))
	_check_selection(out, cat, st)


def test_append_over_a_four_way_split_equals_the_unsplit_selection(driver):
	cat, rng = _random_catalog()
	st = _random_stamps(rng, 203)       # (no multiple of 4: the runs differ in length)
	st[7] = (400, 420, 600, 640)        # a stamp without stars at a run's start, one at its end
	st[49] = (-80, -60, -90, -70)
	out = driver('\n'.join(_catalog_text(cat) + _select_text(st, 1) + _select_text(st, 4)))
	assert out[:7] == out[7:]
	_check_selection(out[:7], cat, st)
	assert _ints(out[0])[-1] > 200      # (the case selects stars at all)


# ---- layouts ------------------------------------------------------------------------------------------------------------------
_SHAPES = [(1, 1, 1, 1, 1), (7, 13, 5, 5, 20), (3, 1300, 15, 15, 1), (2500, 1300, 15, 15, 40000)]


@pytest.mark.parametrize('m,T,H,W,cap', _SHAPES)
def test_block_layout_equals_packed_block_layout_and_the_table_of_collect(driver, m, T, H, W, cap):
	got = _ints(driver('block %d %d %d %d %d' % (m, T, H, W, cap))[0])
	layout, nbytes = comm.packed_block_layout(m, T, H, W, n_cat=cap, extras=True)
	names = ('lc', 'contamination', 'status', 'flags', 'mask', 'cat_in_mask', 'sumimage', 'diagnostics')
	assert tuple(layout) == names
	assert got == [layout[k][0] for k in names] + [nbytes]
	# the table FramesJob.collect walks, with its rule for the offsets
	off, offs = 0, []
	for (name, shape, dtype, size), want in zip(comm.frames_block_fields(m, T, H, W, cap), names):
		assert name == want and (shape, dtype) == layout[name][1:] and size == int(np.prod(shape)) * np.dtype(dtype).itemsize
		offs.append(off)
		off = -(-(off + size) // 256) * 256
	assert got == offs + [off]


@pytest.mark.parametrize('m,T,H,W,cap', _SHAPES)
def test_meta_layout_equals_the_fields_of_aperture_batch(driver, m, T, H, W, cap):
	# the sizes of the `fields` of pipeline.ApertureBatch, in its order, and its loop over them
	sizes = [T * 4, T * 8, m * 4 * 4, (m + 1) * 8, cap * 8, cap * 4, cap * 4, cap * 4, cap * 4, cap * 4, m * 8, m * 8, m * 8, m * 8]
	offs, total = [], 0
	for nbytes in sizes:
		offs.append(total)
		total = -(-(total + max(nbytes, 16)) // 256) * 256
	assert _ints(driver('meta %d %d %d' % (T, m, cap))[0]) == offs + [total]


def test_meta_layout_of_an_empty_catalogue(driver):
	got = _ints(driver('meta 13 7 0')[0])
	assert got[:5] == [0, 256, 512, 768, 1024] and got[5] == 1280 and got[-1] == 14 * 256


# ---- the per-target decision ----------------------------------------------------------------------------------------------------
_CODE_OF_TEXT = {v: k for k, v in pipeline._EVENT_TEXT.items()}


class _Recorder(object):
	def __init__(self):
		self.codes = []

	def error(self, msg):
		self.codes.append(_CODE_OF_TEXT['ERROR: ' + msg])

	def warning(self, msg):
		self.codes.append(_CODE_OF_TEXT['WARNING: ' + msg])


def _plugin_decision(flags, status, stamp, limits, attempts_left, budget, mask, sumimage):
	"""One turn of the loop of plugins.AperturePhotometry.do_photometry on plain data: (outcome, status, moved, stamp, kind, edge_flux or
	None, codes) with outcome 0 stands, 1 error, 2 resize."""
	log = _Recorder()
	attempts_left -= 1
	try:
		if plugins.mask_outcome(flags, log) == 'error':
			return 1, 2, 0, stamp, 0, None, log.codes
	except RuntimeError as e:
		assert str(e) == plugins._MASK_EXCEPTIONS[flags >> 8]
		return 1, 2, 0, stamp, flags >> 8, None, log.codes + [5]
	wanted = stamps.edge_requests(flags)
	if wanted:
		grown = list(stamp)
		for name, _bit, idx, sign in stamps.SIDES:
			grown[idx] += sign * wanted.get(name, 0)
		after = stamps.clip_stamp(grown, limits)
		if after == tuple(stamp):
			log.warning('Could not resize stamp any further.')
		else:
			flux = None
			if not np.isnan(budget):
				flux = stamps.quick_break_flux(sumimage, mask, stamp, after, wanted)
				assert (flux is None) == (not stamps.stuck_sides(stamp, after, wanted))
				if flux is not None and flux > budget:
					log.error('Stamp resize hit limit. Haloswitch quick break.')
					return 1, 2, 1, after, 0, flux, log.codes
			if attempts_left == 0:
				log.error('Too many stamp resizes.')
				return 1, 2, 1, after, 0, flux, log.codes
			return 2, 0, 1, after, 0, flux, log.codes
	if flags >> 8 == 6:
		log.error('No targets in mask.')
	return 0, status, 0, stamp, 0, None, log.codes


def _decide_text(flags, status, stamp, limits, attempts_left, budget, mask, sumimage):
	H, W = mask.shape
	return 'decide %d %d %s %s %d %s %d %d\n%s\n%s' % (flags, status, ' '.join(map(str, stamp)), ' '.join(map(str, limits)), attempts_left,
		_hex64(budget), H, W, ' '.join(str(int(v)) for v in mask.ravel()), _hex64(sumimage))


def _check_decisions(driver, cases):
	out = driver('\n'.join(_decide_text(*c) for c in cases))
	assert len(out) == len(cases)
	outcomes = set()
	for line, c in zip(out, cases):
		got = line.split()
		outcome, status, moved, after, kind, flux, codes = _plugin_decision(*c)
		assert [int(v) for v in got[:7]] == [outcome, status, moved] + list(after), (c[:6], line)
		assert int(got[7]) == kind, (c[:6], line)
		if flux is not None:
			assert int(got[8], 16) == int(np.float64(flux).view('uint64')), (c[:6], line)
		assert [int(v) for v in got[10:]] == codes and int(got[9]) == len(codes), (c[:6], line)
		outcomes.add((outcome, tuple(codes)))
	return outcomes


_STAMP = (50, 55, 60, 64)
#: the region around _STAMP: interior, the stamp at each limit, less than a resize step from every limit, at all four
_LIMITS = [(0, 200, 0, 200), (50, 200, 0, 200), (0, 55, 0, 200), (0, 200, 60, 200), (0, 200, 0, 64), (45, 58, 57, 66), (50, 55, 60, 64)]


def _image(seed, nan_edges=False):
	rng = np.random.default_rng(seed)
	mask = rng.random((5, 4)) < 0.7
	mask[0, 1] = mask[-1, 2] = mask[2, 0] = mask[3, -1] = True
	sumimage = rng.uniform(1.0, 1e5, (5, 4))
	if nan_edges:
		sumimage[0, 1] = sumimage[-1, 0] = sumimage[1, 0] = sumimage[2, -1] = sumimage[-1, -1] = np.nan
		mask[-1, 0] = mask[1, 0] = mask[2, -1] = True
	return mask.astype('uint8'), sumimage


def _budgets(flags, limits, mask, sumimage, stamp=_STAMP):
	"""NaN (not a bright target), and a budget below, at and above the flux on the stuck edges (where there are any)."""
	wanted = stamps.edge_requests(flags)
	grown = list(stamp)
	for name, _bit, idx, sign in stamps.SIDES:
		grown[idx] += sign * wanted.get(name, 0)
	flux = stamps.quick_break_flux(sumimage, mask, stamp, stamps.clip_stamp(grown, limits), wanted) if wanted else None
	flux = 1000.0 if flux is None else flux
	return [np.nan, 0.5 * flux, flux, 2.0 * flux]


def test_decision_equals_the_plugin_edges_limits_attempts_budgets(driver):
	cases = []
	for nan_edges in (False, True):
		mask, sumimage = _image(3, nan_edges)
		for edges, limits, attempts in itertools.product(range(0, 32, 2), _LIMITS, (1, 2)):
			for budget in _budgets(edges, limits, mask, sumimage):
				cases.append((edges, 1, _STAMP, limits, attempts, budget, mask, sumimage))
	outcomes = _check_decisions(driver, cases)
	assert {(0, ()), (0, (6,)), (1, (7,)), (1, (8,)), (2, ())} == outcomes


def test_decision_equals_the_plugin_flag_bits_and_kinds(driver):
	cases = []
	mask, sumimage = _image(4)
	k = 0
	for edges, bits, kind in itertools.product(range(0, 32, 2), itertools.product((0, 1), (0, 32), (0, 64)), range(8)):
		flags = edges | sum(bits) | (kind << 8)
		limits, attempts = _LIMITS[(k // 8) % len(_LIMITS)], 1 + (k // 3) % 2      # (k % 8 is the kind, 7 -- the empty KDE sample -- included)
		budget = _budgets(flags, limits, mask, sumimage)[(k + k // 8) % 4]           # (... and every kind meets every budget)
		cases.append((flags, 3 if flags & 1 else 1, _STAMP, limits, attempts, budget, mask, sumimage))
		k += 1
	outcomes = _check_decisions(driver, cases)
	assert {c for _o, codes in outcomes for c in codes} == set(range(1, 10))


def test_decision_one_pixel_stamp_and_the_retry_limits(driver):
	mask, sumimage = np.ones((1, 1), dtype='uint8'), np.array([[250.0]])
	cases = []
	for edges, limits in itertools.product(range(0, 32, 2), [(0, 200, 0, 200), (10, 11, 20, 21), (10, 200, 0, 21), (0, 11, 20, 200)]):
		for attempts in (1, 2, stamps.retry_limit(5.0), stamps.retry_limit(7.0)):
			for budget in (np.nan, 100.0, 250.0, 1000.0):
				cases.append((edges, 1, (10, 11, 20, 21), limits, attempts, budget, mask, sumimage))
	cases.append((2 | 8, 1, (10, 11, 20, 21), (10, 200, 0, 21), 2, 100.0, mask, np.array([[np.nan]])))
	outcomes = _check_decisions(driver, cases)
	assert (1, (7,)) in outcomes and (2, ()) in outcomes


# ---- numpy's pairwise sum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 7, 8, 9, 127, 128, 129, 1000, 4099])
def test_pairwise_sum_equals_numpy(driver, n):
	rng = np.random.default_rng(n)
	a = 10.0**rng.uniform(-8, 8, n) * rng.choice([-1.0, 1.0], n)
	b = 10.0**rng.uniform(-8, 8, n)
	out = driver('pairwise %d %s\npairwise %d %s' % (n, _hex64(a), n, _hex64(b)))
	assert [int(v, 16) for v in out] == [int(np.float64(np.add.reduce(x)).view('uint64')) for x in (a, b)]
	if n:
		assert float(np.nansum(b)) == float(np.add.reduce(b))


# ---- the round planner ----------------------------------------------------------------------------------------------------------
def _per_target(H, W, T, cubes):
	pitch = -(-T // 32) * 32
	return (3.0 * H * W * pitch * 4 if cubes else 0.0) + 5.0 * T * 8 + float(H * W) * 13 + 256


def _plan(driver, st, T, cubes, budget):
	out = driver('plan %d %d %s %d\n%s' % (T, int(cubes), _hex64(budget), len(st), '\n'.join(' '.join(str(int(v)) for v in s) for s in st)))
	assert out[0].split()[0] == 'parts'
	parts, k = [], 1
	for _p in range(int(out[0].split()[1])):
		n_pieces = int(out[k].split()[1])
		assert out[k].split()[0] == 'part'
		pieces = []
		for line in out[k + 1:k + 1 + n_pieces]:
			w = line.split()
			assert w[0] == 'piece' and int(w[4]) == len(w) - 5
			pieces.append((int(w[1]), int(w[2]), float(np.array(int(w[3], 16), dtype='uint64').view('float64')), [int(v) for v in w[5:]]))
		parts.append(pieces)
		k += 1 + n_pieces
	assert k == len(out)
	return parts


def _planner_stamps():
	rng = np.random.default_rng(5)
	sizes = [(15, 15)] * 40 + [(25, 15)] * 9 + [(15, 25)] * 7 + [(35, 35)] * 3 + [(100, 3)] + [(15, 15)] * 11
	st = []
	for h, w in sizes:
		r, c = int(rng.integers(0, 500)), int(rng.integers(0, 500))
		st.append((r, r + h, c, c + w))
	return np.asarray(st, dtype='int64')


@pytest.mark.parametrize('cubes', [False, True])
@pytest.mark.parametrize('share', ['whole round', 'half a group', 'less than one target'])
def test_planner_pieces_cover_the_round_under_the_budget(driver, share, cubes):
	st, T = _planner_stamps(), 70
	h, w = st[:, 1] - st[:, 0], st[:, 3] - st[:, 2]
	need = np.array([_per_target(a, b, T, cubes) for a, b in zip(h, w)])
	budget = {'whole round': 2.0 * need.sum(), 'half a group': 25.5 * _per_target(15, 15, T, cubes), 'less than one target': 0.5 * need.min()}[share]
	parts = _plan(driver, st, T, cubes, budget)
	seen = []
	for part in parts:
		assert part
		for H, W, nbytes, idx in part:
			assert idx == sorted(idx) and len(set(idx)) == len(idx) and idx      # ascending target index
			assert all((h[i], w[i]) == (H, W) for i in idx)                    # one stamp size
			assert nbytes == _per_target(H, W, T, cubes) * len(idx)
			seen += idx
		total = sum(p[2] for p in part)
		assert total <= budget or (len(part) == 1 and len(part[0][3]) == 1)
	assert sorted(seen) == list(range(len(st)))                                # every target in exactly one piece
	keys = [H * 100000 + W for part in parts for H, W, _n, _i in part]
	assert keys == sorted(keys)
	if share == 'whole round':
		# the groups of the round and their order: by size key h * 100000 + w, ascending, targets in ascending order
		by_size = {}
		for i in range(len(st)):
			by_size.setdefault(int(h[i]) * 100000 + int(w[i]), []).append(i)
		assert len(parts) == 1
		assert [(H, W, idx) for H, W, _n, idx in parts[0]] == [(k // 100000, k % 100000, by_size[k]) for k in sorted(by_size)]
	elif share == 'half a group':
		assert [len(i) for part in parts for H, W, _n, i in part if (H, W) == (15, 15)] == [25, 25, 1]
	else:
		assert all(len(part) == 1 and len(part[0][3]) == 1 for part in parts)


# ---- the size classes of the page-locked pool -----------------------------------------------------------------------------------
def test_size_class_monotone_and_the_known_values(driver):
	ns = sorted(set([1, 2, 65535, 65536, 65537, 1 << 20, (1 << 20) + 1, 3 << 20, (3 << 20) + 1, 1 << 30, (1 << 33) + 5]
		+ [int(v) for v in 2.0**np.random.default_rng(1).uniform(0, 34, 400)]))
	got = _ints(driver('size_class %d %s' % (len(ns), ' '.join(map(str, ns))))[0])
	assert all(c >= n for c, n in zip(got, ns))
	assert got == sorted(got)
	known = {1: 65536, 65536: 65536, 65537: 131072, 1 << 20: 1 << 20, (1 << 20) + 1: (1 << 20) + (1 << 17), 3 << 20: 3 << 20}
	assert {n: c for n, c in zip(ns, got) if n in known} == known
