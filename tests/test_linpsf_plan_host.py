# -*- coding: utf-8 -*-
"""
CPU check of the LinPSF plan's device-free rules (photometry_amd/csrc/linpsf_plan_rules.h): the header compiled for the host with
AddressSanitizer and UBSan into the driver tests/hostsim/linpsf_plan_host.cpp, which composes the rules serially into the plan of a
target, and held to the Python restatement of the plan kernel in ``linpsf_common`` (``plan_class``, ``segments``, ``union_plan``,
``intervals_visited``, ``on_stamp``): class, segments and their contents, the union list and its keys, the tile masks, the item
offsets -- for every SPOC row of ``linpsf_common.CASES`` on both paths, and for hand cases at the edges of the rules.
"""
import os
import subprocess
import numpy as np
import pytest
import conftest
import linpsf_common as lc

SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'linpsf_plan_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'linpsf_plan_host')

POLY, DIRECT, MATRIX, MANY = 0, 1, 2, 3
_CLS = {'poly': POLY, 'direct': DIRECT, 'matrix': MATRIX, 'many': MANY}


@pytest.fixture(scope='module')
def driver():
	os.makedirs(OUT_DIR, exist_ok=True)
	subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall',
		'-I' + os.path.join(conftest.ROOT, 'photometry_amd', 'csrc'), '-o', OUT, SRC], check=True)

	def run(text):
		r = subprocess.run([OUT], input=text, capture_output=True, text=True, timeout=120)
		assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
		assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
		assert r.stderr == '', r.stderr
		return r.stdout.splitlines()
	return run


def _hex64(values):
	return ['%016x' % v for v in np.asarray(values, dtype='float64').ravel().view('uint64')]


def _target_text(t):
	"""One ``target`` command: ``t`` holds H, W, cutoff, path and the ``(S, T)`` arrays valid, ax, by, rows, cols."""
	S, T = t['rows'].shape
	words = ['target', str(t['H']), str(t['W']), _hex64(t['cutoff'])[0], str(t['path']), str(S), str(T)]
	per = np.stack((t['valid'].astype('int64').astype(str).ravel(), t['ax'].astype('int64').astype(str).ravel(), t['by'].astype('int64').astype(str).ravel(),
		np.array(_hex64(t['rows'])), np.array(_hex64(t['cols']))), axis=1)
	return ' '.join(words) + '\n' + '\n'.join(' '.join(r) for r in per)


def _parse(lines):
	"""The driver's answer as one dict per target."""
	out, cur = [], None
	for line in lines:
		w = line.split()
		assert w[0] != 'FAILED:', line
		if w[0] == 'path':
			cur = {'path': int(w[1]), 'stars': [], 'segments': [], 'segstars': [], 'kdoubles': [], 'koff': [], 'tiles': [], 'edge_tiles': []}
		elif w[0] == 'star':
			cur['stars'].append(dict(zip(('nc', 'axmin', 'bymin', 'nby', 'jmin', 'jmax', 'imin', 'imax', 'item_off'), map(int, w[2:]))))
		elif w[0] == 'seg':
			cur['segments'].append((int(w[1]), int(w[2])))
			cur['kdoubles'].append(int(w[3]))
			cur['koff'].append(int(w[4]))
			cur['segstars'].append([])
		elif w[0] == 'segstar':
			cur['segstars'][-1].append(dict(zip(('axmin', 'bymin', 'na', 'nb', 'ksub'), map(int, w[1:]))))
		elif w[0] in ('nseg', 'npix', 'items'):
			cur[w[0]] = int(w[1])
		elif w[0] in ('keys', 'ulist', 'usig', 'ckeys', 'corder'):
			cur[w[0]] = [int(v) for v in w[1:]]
		elif w[0] == 'tiles':
			cur['tiles'].append(int(w[2]))
			cur['edge_tiles'].append(int(w[3]))
		elif w[0] == 'end':
			out.append(cur)
			cur = None
		else:
			raise AssertionError(line)
	assert cur is None
	return out


def _plans(driver, targets):
	got = _parse(driver('\n'.join(_target_text(t) for t in targets)))
	assert len(got) == len(targets)
	return got


def _from_positions(model, pos_rows, pos_cols, H, W, path, cutoff=lc.CUTOFF):
	"""The driver's input of a target at these positions: the origins come from ``lc.axis_origin``."""
	ax, _, vx = lc.axis_origin(model.tx, pos_cols)
	by, _, vy = lc.axis_origin(model.ty, pos_rows)
	return {'H': H, 'W': W, 'cutoff': float(cutoff), 'path': path, 'valid': vx & vy, 'ax': ax, 'by': by, 'rows': np.asarray(pos_rows, dtype='float64'),
		'cols': np.asarray(pos_cols, dtype='float64')}


def _popcount(v):
	return bin(v).count('1')


def _check_boxes(got, t):
	"""``nc`` and the pixel box of every star, the item offsets of a polynomial target: from the inputs, literally."""
	items = 0
	for s, q in enumerate(got['stars']):
		ok = t['valid'][s]
		box = None
		if ok.any():
			jmin, jmax = max(int(np.floor(t['cols'][s][ok] - t['cutoff']).min()), 0), min(int(np.ceil(t['cols'][s][ok] + t['cutoff']).max()), t['W'] - 1)
			imin, imax = max(int(np.floor(t['rows'][s][ok] - t['cutoff']).min()), 0), min(int(np.ceil(t['rows'][s][ok] + t['cutoff']).max()), t['H'] - 1)
			if jmin <= jmax and imin <= imax:
				box = (jmin, jmax, imin, imax)
		if box is None:
			assert (q['nc'], q['axmin'], q['bymin'], q['nby'], q['jmin'], q['jmax'], q['imin'], q['imax']) == (0, 0, 0, 1, 0, -1, 0, -1), (s, q)
		else:
			a, b = t['ax'][s][ok], t['by'][s][ok]
			assert (q['jmin'], q['jmax'], q['imin'], q['imax']) == box, (s, q, box)
			assert (q['axmin'], q['bymin'], q['nby']) == (a.min(), b.min(), b.max() - b.min() + 1), (s, q)
			assert q['nc'] == (a.max() - a.min() + 1) * (b.max() - b.min() + 1), (s, q)
		if got['path'] == POLY:
			assert q['item_off'] == items, (s, q, items)
			if box is not None:
				items += q['nc'] * (box[1] - box[0] + 1) * (box[3] - box[2] + 1)
	assert got['items'] == (items if got['path'] == POLY else -1)


def _check_cadence_order(got, t):
	"""The sort key of every cadence of a polynomial target, literally: the stars' origin numbers inside their boxes (0 where the
	position is not valid or the star has no origins) as digits to the base ``MAX_ORIGINS + 1``, the first star the most significant, then
	the cadence in the low 13 bits; and the cadences read back from the sorted keys."""
	S, T = t['rows'].shape
	if got['path'] != POLY or T > 8192:
		assert 'ckeys' not in got
		return
	keys = []
	for k in range(T):
		key = 0
		for s, q in enumerate(got['stars']):
			cc = (int(t['ax'][s][k]) - q['axmin']) * q['nby'] + (int(t['by'][s][k]) - q['bymin']) if (t['valid'][s][k] and q['nc'] > 0) else 0
			assert 0 <= cc <= lc.MAX_ORIGINS
			key = key * (lc.MAX_ORIGINS + 1) + cc
		keys.append(key * 8192 + k)
	assert got['ckeys'] == keys and max(keys) < 2**64
	assert got['corder'] == [k & 8191 for k in sorted(keys)] and sorted(got['corder']) == list(range(T))


def _check_segments(got, t):
	"""The contents of every segment from the inputs: first interval and count per axis over the segment's valid cadences, ``ksub`` and
	``kdoubles`` from the tile masks, ``koff`` as the running sum."""
	S, T = t['rows'].shape
	listed = 0 <= got['npix'] <= lc.MFMA_PIXELS
	koff = 0
	for (t0, t1), stars, kd, ko in zip(got['segments'], got['segstars'], got['kdoubles'], got['koff']):
		blocks = 0
		for s, g in enumerate(stars):
			ok = t['valid'][s][16 * t0:min(16 * t1, T)]
			if got['stars'][s]['nc'] > 0 and ok.any():
				a, b = t['ax'][s][16 * t0:min(16 * t1, T)][ok], t['by'][s][16 * t0:min(16 * t1, T)][ok]
				want = (a.min(), b.min(), a.max() - a.min() + 1, b.max() - b.min() + 1)
			else:
				want = (0, 0, 0, 0)
			assert (g['axmin'], g['bymin'], g['na'], g['nb']) == want, (t0, t1, s, g, want)
			assert g['na'] <= lc.MFMA_SPAN and g['nb'] <= lc.MFMA_SPAN
			if listed:
				assert g['ksub'] == blocks, (t0, t1, s, g, blocks)
				if g['na'] > 0:
					blocks += _popcount(got['tiles'][s]) * lc.mfma_steps(g['na'], g['nb'])
		if listed:
			assert (kd, ko) == (64 * blocks, koff), (t0, t1, kd, ko, blocks, koff)
			koff += 64 * blocks
	assert got['nseg'] == len(got['segments']) <= lc.MFMA_SEGS
	assert [a for a, _ in got['segments'][1:]] == [b for _, b in got['segments'][:-1]]        # they tile the series
	if got['segments']:
		assert got['segments'][0][0] == 0 and got['segments'][-1][1] == (T + 15) // 16


def _check_union(got, t):
	"""The union list against ``lc.union_plan``: the keys, the order of the list, the membership bytes, the tile masks."""
	n_pix, tiles, keys = lc.union_plan(t['rows'], t['cols'], t['H'], t['W'], t['cutoff'], with_keys=True)
	assert got['npix'] == n_pix
	if tiles is None:
		assert 'ulist' not in got and got['path'] != MATRIX
		return
	order = np.argsort(keys)
	assert got['keys'] == keys[order].tolist()
	assert got['ulist'] == (keys[order] & 0xffff).tolist()                     # the pixel, raster index
	assert got['usig'] == (((keys[order] >> 16) & 15) | (((keys[order] >> 20) & 15) << 4)).tolist()
	assert [_popcount(v) for v in got['tiles']] == tiles
	for s in range(len(tiles)):
		member = [r >> 4 for r, b in enumerate(got['usig']) if (b >> s) & 1]
		edge = [r >> 4 for r, b in enumerate(got['usig']) if (b >> (4 + s)) & 1]
		assert got['tiles'][s] == sum(1 << r for r in set(member)) and got['edge_tiles'][s] == sum(1 << r for r in set(edge))
		assert set(edge) <= set(member)


def _check_against_plan_class(got, want, t):
	assert got['path'] == _CLS[want['cls']], (got['path'], want)
	if want['cls'] == 'many':
		return
	assert [q['nc'] for q in got['stars']] == want['origins']
	_check_boxes(got, t)
	_check_cadence_order(got, t)
	segs = want.get('segments')
	assert got['segments'] == (segs or [])
	_check_segments(got, t)
	if not segs:
		assert got['npix'] == -1
		return
	assert got['npix'] == want['n_pix']
	_check_union(got, t)
	if 'shapes' in want:
		assert [[(g['na'], g['nb']) for g in stars] for stars in got['segstars']] == want['shapes']
		assert [_popcount(v) for v in got['tiles']] == want['tiles']
		assert [8 * kd for kd in got['kdoubles']] == want['lds']


SPOC_ROWS = [n for n, r in lc.CASES.items() if r.get('kind', 'spoc') == 'spoc' and r.get('cutoff', 5) is not None]


def test_constants_equal_the_restated_ones(driver):
	out = driver('constants')
	assert [int(v) for v in out[0].split()[1:]] == [lc.MAX_STARS, lc.MFMA_STARS, lc.MFMA_PIXELS, lc.MFMA_SPAN, lc.MFMA_SEGS, lc.MFMA_CAD_TILES,
		lc.MFMA_LDS_SMALL, lc.MFMA_LDS_LARGE, lc.MAX_ORIGINS]
	assert [int(v) for v in out[1].split()[1:]] == [lc.mfma_steps(1, 1), lc.mfma_steps(2, 2), lc.mfma_steps(3, 3), lc.mfma_steps(3, 2)]


@pytest.mark.parametrize('name', SPOC_ROWS)
def test_row_plans_equal_plan_class(driver, name):
	"""Every target of the row on both paths: class, ``nc``, segments, shapes, ``n_pix``, tiles and LDS equal ``lc.plan_class``; the
	union list is ordered by ``union_plan``'s keys; boxes, segment contents and item offsets follow from the inputs."""
	case = lc.build_case(name)
	_, model = lc.prf_and_model('spoc')
	s, so = case['scene'], case['star_offsets']
	classes = set()
	for path in (0, 1):
		targets = [_from_positions(model, case['pos_row'][so[i]:so[i + 1]], case['pos_col'][so[i]:so[i + 1]], s.height, s.width, path) for i in range(s.n_targets)]
		got = _plans(driver, targets)
		for i, t in enumerate(targets):
			want = lc.plan_class(model, t['rows'], t['cols'], s.height, s.width, path)
			_check_against_plan_class(got[i], want, t)
			classes.add((path, want['cls']))
	assert {c for p, c in classes if p == 0} <= {'poly', 'direct', 'many'}         # the vector-ALU path makes no matrix-core plan


# ---- hand cases at the edges of the rules: the origins are given, not derived from a position ---------------------------------------
def _hand(S, T, H=11, W=11, path=1, pos=None):
	"""``S`` stars standing at ``pos[s]`` (the stamp's centre by default), every cadence valid at origin (0, 0)."""
	t = {'H': H, 'W': W, 'cutoff': lc.CUTOFF, 'path': path, 'valid': np.ones((S, T), dtype=bool), 'ax': np.zeros((S, T), dtype='int64'),
		'by': np.zeros((S, T), dtype='int64'), 'rows': np.empty((S, T)), 'cols': np.empty((S, T))}
	for s in range(S):
		t['rows'][s], t['cols'][s] = pos[s] if pos else ((H - 1) / 2.0 + 0.2 * s, (W - 1) / 2.0 - 0.3 * s)
	return t


def _check_hand(got, t):
	_check_boxes(got, t)
	_check_cadence_order(got, t)
	_check_segments(got, t)
	if got['segments']:
		_check_union(got, t)


def test_a_star_never_valid_and_a_star_never_on_the_stamp(driver):
	never_valid = _hand(2, 20)
	never_valid['valid'][1] = False
	never_valid['rows'][1] = never_valid['cols'][1] = np.nan
	off_stamp = _hand(2, 20, pos=[(5.0, 5.0), (45.0, 5.2)])
	half_valid = _hand(2, 20)                    # no valid position in the second tile of cadences
	half_valid['valid'][1, 16:] = False
	for t, shapes in ((never_valid, [(1, 1), (0, 0)]), (off_stamp, [(1, 1), (0, 0)]), (half_valid, [(1, 1), (1, 1)])):
		got = _plans(driver, [t])[0]
		assert got['path'] == MATRIX and got['segments'] == [(0, 2)]
		assert [(g['na'], g['nb']) for g in got['segstars'][0]] == shapes
		assert (got['stars'][1]['nc'] == 0) == (shapes[1] == (0, 0))
		assert (got['tiles'][1] == 0) == (shapes[1] == (0, 0)) and got['tiles'][0] != 0
		_check_hand(got, t)
	assert _plans(driver, [never_valid])[0]['stars'][1]['jmax'] == -1 and _plans(driver, [off_stamp])[0]['stars'][1]['imax'] == -1


def test_span_of_exactly_three_intervals_and_of_four(driver):
	k = np.arange(32)
	three, four, four_over_two_tiles = _hand(1, 16), _hand(1, 16), _hand(1, 32)
	three['by'][0] = k[:16] % lc.MFMA_SPAN
	four['ax'][0] = k[:16] % (lc.MFMA_SPAN + 1)
	four_over_two_tiles['ax'][0] = np.where(k < 16, k % 3, 3)
	got = _plans(driver, [three, four, four_over_two_tiles])
	assert got[0]['path'] == MATRIX and got[0]['segments'] == [(0, 1)] and (got[0]['segstars'][0][0]['na'], got[0]['segstars'][0][0]['nb']) == (1, 3)
	# four intervals inside ONE tile of cadences: no segments, and with 4 origins the polynomial fit
	assert got[1]['path'] == POLY and got[1]['segments'] == [] and got[1]['stars'][0]['nc'] == 4 and got[1]['npix'] == -1
	assert got[2]['path'] == MATRIX and got[2]['segments'] == [(0, 1), (1, 2)]
	assert [(g[0]['axmin'], g[0]['na']) for g in got[2]['segstars']] == [(0, 3), (3, 1)]
	for g, t in zip(got, (three, four, four_over_two_tiles)):
		_check_hand(g, t)


def test_eight_segments_and_nine(driver):
	def stairs(n, both):
		t = _hand(2, 16 * n - 5)
		t['ax'][:] = 3 * (np.arange(16 * n - 5) // 16)
		if both:
			t['by'][1] = 3 * (np.arange(16 * n - 5) // 16)
		return t
	eight, nine, nine_many_origins = stairs(lc.MFMA_SEGS, False), stairs(lc.MFMA_SEGS + 1, False), stairs(lc.MFMA_SEGS + 1, True)
	got = _plans(driver, [eight, nine, nine_many_origins])
	assert got[0]['path'] == MATRIX and got[0]['segments'] == [(q, q + 1) for q in range(8)]
	assert [g[1]['axmin'] for g in got[0]['segstars']] == [3 * q for q in range(8)] and got[0]['koff'] == [q * got[0]['kdoubles'][0] for q in range(8)]
	# a ninth segment: the vector ALUs -- the polynomial fit with 25 origins, the direct kernel with 25 x 25
	assert (got[1]['path'], got[1]['segments'], got[1]['stars'][1]['nc']) == (POLY, [], 25)
	assert (got[2]['path'], got[2]['segments'], got[2]['stars'][1]['nc']) == (DIRECT, [], 625) and got[2]['items'] == -1
	assert lc.MAX_ORIGINS == 36 and got[1]['items'] > 0
	for g, t in zip(got, (eight, nine, nine_many_origins)):
		_check_hand(g, t)
	# 36 origins are not too many, 37 are
	for n, want in ((36, POLY), (37, DIRECT)):
		t = _hand(1, 48, path=0)
		t['ax'][0] = np.arange(48) % n
		assert _plans(driver, [t])[0]['path'] == want


def test_stamp_of_65535_pixels_and_of_65536(driver):
	pos = [(100.3, 100.2)]
	got = _plans(driver, [_hand(1, 20, H=255, W=257, pos=pos), _hand(1, 20, H=256, W=256, pos=pos)])
	assert got[0]['path'] == MATRIX and got[0]['segments'] == [(0, 2)] and 0 < got[0]['npix'] <= lc.MFMA_PIXELS
	assert got[1]['path'] == POLY and got[1]['segments'] == [] and got[1]['npix'] == -1
	_check_hand(got[0], _hand(1, 20, H=255, W=257, pos=pos))
	_check_hand(got[1], _hand(1, 20, H=256, W=256, pos=pos))


def test_series_of_4096_cadences_and_of_4097(driver):
	got = _plans(driver, [_hand(2, 16 * lc.MFMA_CAD_TILES), _hand(2, 16 * lc.MFMA_CAD_TILES + 1)])
	assert got[0]['path'] == MATRIX and got[0]['segments'] == [(0, lc.MFMA_CAD_TILES)]
	assert got[1]['path'] == POLY and got[1]['segments'] == []
	# the rows of the table that are built for this: one segment of 256 tiles on the matrix cores, none a cadence later
	_, model = lc.prf_and_model('spoc')
	for name, cls in (('cadences_4096', 'matrix'), ('cadences_4097', 'poly')):
		case = lc.build_case(name)
		assert [c['cls'] for c in lc.case_classes(case, 1)] == [cls, cls]


def test_union_list_of_255_pixels_and_of_257(driver):
	_, model = lc.prf_and_model('spoc')
	for name, n_pix, path in (('union_under', 255, MATRIX), ('union_over', 257, DIRECT)):
		case = lc.build_case(name)
		so = case['star_offsets']
		for i in range(case['scene'].n_targets):
			t = _from_positions(model, case['pos_row'][so[i]:so[i + 1]], case['pos_col'][so[i]:so[i + 1]], 21, 21, 1)
			got = _plans(driver, [t])[0]
			assert (got['npix'], got['path'], len(got['segments'])) == (n_pix, path, 3)
			assert ('ulist' in got) == (n_pix <= lc.MFMA_PIXELS)


def test_union_list_of_exactly_256_pixels_and_of_272(driver):
	"""A cut-off that reaches every pixel: the 256 pixels of a 16 x 16 stamp are a full list on the matrix cores, one more column is not."""
	full, over = _hand(2, 20, H=16, W=16), _hand(2, 20, H=16, W=17)
	full['cutoff'] = over['cutoff'] = 30.0
	got = _plans(driver, [full, over])
	assert (got[0]['npix'], got[0]['path']) == (lc.MFMA_PIXELS, MATRIX) and got[0]['ulist'] == list(range(256)) and got[0]['tiles'] == [0xffff, 0xffff]
	assert (got[1]['npix'], got[1]['path'], got[1]['segments']) == (272, POLY, [(0, 2)]) and 'ulist' not in got[1]
	_check_hand(got[0], full)
	_check_hand(got[1], over)


def test_cadence_keys_of_a_two_star_target(driver):
	"""Two stars over 2 x 3 and 3 x 1 origins, an invalid cadence, a star without origins: the keys by hand."""
	T = 40
	k = np.arange(T)
	t = _hand(3, T, path=0, pos=[(5.0, 5.0), (5.3, 4.6), (45.0, 5.0)])
	t['ax'][0], t['by'][0] = 7 + k % 2, -4 + (k // 2) % 3
	t['ax'][1], t['by'][1] = -2 + (k // 5) % 3, 9
	t['ax'][2] = k % 4                                  # never on the stamp: digit 0 whatever its origins
	t['valid'][1, 11] = False
	got = _plans(driver, [t])[0]
	assert got['path'] == POLY and [q['nc'] for q in got['stars']] == [6, 3, 0]
	digit0, digit1 = (k % 2) * 3 + (k // 2) % 3, (k // 5) % 3
	digit1[11] = 0
	assert got['ckeys'] == (((digit0 * 37 + digit1) * 37 + 0) * 8192 + k).tolist()
	assert got['corder'] == sorted(range(T), key=lambda c: (digit0[c], digit1[c], c))
	_check_hand(got, t)
