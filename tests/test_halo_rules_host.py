# -*- coding: utf-8 -*-
"""
CPU check of Halo photometry's device-free rules (photometry_amd/csrc/halo_rules.h): the header compiled for the host with
AddressSanitizer and UBSan into the driver tests/hostsim/halo_rules_host.cpp and held to numpy, to ``photometry_amd.halo`` and to the
restatement ``halo_common``: (a) the order-preserving keys and the radix selection composed serially from the pass rules, (b) the
pixel rule ``drop_pixel`` of the frames path against ``nanmedian(float64) < minflux``, (c) the host tables of the entries and their
argument checks, (d) the optimiser's state machine -- the whole L-BFGS run serially by the driver with every transition taken from
the header, against ``halo_common.lbfgs``, and hand cases driven by scripted numbers.
"""
import os
import subprocess
import warnings
import numpy as np
import pytest
import conftest
import halo_common as hc
from photometry_amd import halo

SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'halo_rules_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'halo_rules_host')

MINFLUX = -100.0


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
		assert 'FAILED:' not in r.stdout, r.stdout[-2000:]
		return r.stdout.splitlines()
	return run


def _hex64(values):
	return ['%016x' % v for v in np.asarray(values, dtype='float64').ravel().view('uint64')]


def _hex32(values):
	return ['%08x' % v for v in np.asarray(values, dtype='float32').ravel().view('uint32')]


def _f64(word):
	return np.array([int(word, 16)], dtype='uint64').view('float64')[0]


def test_header_compiles_alone(tmp_path):
	src = tmp_path / 'only.cpp'
	src.write_text('#include "halo_rules.h"\n#include "linpsf_plan_rules.h"\nint main() { return tp_halo::mid_lo(3) - 1; }\n')
	subprocess.run(['g++', '-std=c++17', '-Wall', '-fsyntax-only', '-I' + os.path.join(conftest.ROOT, 'photometry_amd', 'csrc'), str(src)], check=True)


# ---- (a) keys and selection -----------------------------------------------------------------------------------------------------
def _key_values(dtype):
	fi = np.finfo(dtype)
	one = dtype(1.0)
	hand = [0.0, -0.0, np.inf, -np.inf, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max, -fi.max, 1.0, -1.0,
		np.nextafter(one, dtype(2)), np.nextafter(one, dtype(0)), np.nextafter(-one, dtype(-2)), np.nextafter(-one, dtype(0)), MINFLUX,
		np.nextafter(dtype(MINFLUX), dtype(0)), np.nextafter(dtype(MINFLUX), dtype(-np.inf))]
	rng = np.random.default_rng(21)
	rnd = rng.normal(size=10000) * 10.0**rng.integers(-30, 30, size=10000)
	with np.errstate(over='ignore', under='ignore'):
		return np.concatenate([np.array(hand, dtype=dtype), rnd.astype(dtype)])


@pytest.mark.parametrize('dtype,cmd,tohex,uint', [(np.float64, 'keys', _hex64, 'uint64'), (np.float32, 'fkeys', _hex32, 'uint32')])
def test_keys_keep_the_order_and_round_trip(driver, dtype, cmd, tohex, uint):
	x = _key_values(dtype)
	out = driver(f'{cmd} {len(x)} ' + ' '.join(tohex(x)))
	keys = np.array([int(line.split()[0], 16) for line in out], dtype=uint)
	back = np.array([int(line.split()[1], 16) for line in out], dtype=uint)
	assert np.array_equal(back, x.view(uint))                                      # the round trip is exact
	order = np.argsort(keys, kind='stable')
	assert np.array_equal(x[order], np.sort(x))                                    # numpy's order (-0 and +0 compare equal there)
	same_key, same_bits = np.diff(keys[order]) == 0, np.diff(x[order].view(uint).astype('int64')) == 0
	assert np.array_equal(same_key, same_bits)
	# strictly: a smaller value has a smaller key, and -0 comes before +0
	assert np.all(keys[order][1:][np.diff(x[order]) > 0] > keys[order][:-1][np.diff(x[order]) > 0])
	assert keys[1] < keys[0]


def _series(kind, n, rng):
	if kind == 'random':
		return rng.uniform(50, 1000, n)
	if kind == 'ties':
		return rng.choice(np.array([3.5, -2.25, 1e-300, 7e8, 3.5000000000000004]), size=n)
	return rng.normal(size=n) * 10.0**rng.integers(-3, 4, size=n)                # mixed sign


@pytest.mark.parametrize('kind', ['random', 'ties', 'mixed'])
def test_serial_radix_selection_equals_the_sorted_series(driver, kind):
	rng = np.random.default_rng(31)
	text, want = [], []
	for n in (1, 2, 3, 255, 256, 257, 1300):
		x = _series(kind, n, rng)
		ks = sorted({0, (n - 1) // 2, n // 2, n - 1})
		text.append(f'select {n} {len(ks)} ' + ' '.join(_hex64(x)) + ' ' + ' '.join(map(str, ks)))
		text.append(f'median {n} ' + ' '.join(_hex64(x)))
		s = np.sort(x)
		want += [(_hex64(s[k])[0], k - int(np.count_nonzero(x < s[k]))) for k in ks] + [(_hex64(np.median(x))[0],)]
	out = driver('\n'.join(text))
	got = [tuple([w[0]] + [int(v) for v in w[1:]]) for w in (line.split() for line in out)]
	assert got == want


# ---- (b) the pixel rule of the frames path ----------------------------------------------------------------------------------------
def numpy_rule(x, minflux=MINFLUX):
	x = np.asarray(x, dtype='float32')
	with warnings.catch_warnings():
		warnings.simplefilter('ignore', RuntimeWarning)
		with np.errstate(invalid='ignore'):
			med = np.nanmedian(x.astype('float64')) if len(x) else np.nan
	return bool(med < minflux)


def drop_pixel(driver, series, minflux=MINFLUX):
	"""``nanmedian(float64(x)) < minflux`` as csrc/halo_rules.h (drop_pixel) decides it, for every series: from the count ``n`` of
	non-NaN values, the count ``c`` of values below ``minflux``, ``a = max{x < minflux}`` and ``b = min{x >= minflux}``, without a sort."""
	text = [f'drop {_hex64(minflux)[0]} {len(series)}'] + [f'{len(x)} ' + ' '.join(_hex32(x)) for x in series]
	out = driver('\n'.join(text))
	return [bool(int(v)) for v in out[0].split()]


def _hand_cases():
	below, above = np.nextafter(np.float32(MINFLUX), np.float32(-np.inf)), np.nextafter(np.float32(MINFLUX), np.float32(np.inf))
	cases = [[], [np.nan], [np.nan] * 4, [MINFLUX], [MINFLUX] * 2, [MINFLUX] * 5, [below], [above], [-150, MINFLUX], [-150, -50], [-150, -50.5],
		[-120, -80], [-120, -79.99], [-120.01, -80], [below, MINFLUX], [below, above], [-200, -150, -50, 10], [-200, -150, -100, 10],
		[-200, -100.5, -99.5, 10], [-200, -100.5, -99.25, 10], [-200, -100.75, -99.5, 10], [np.inf], [-np.inf], [np.inf, -np.inf],
		[-np.inf, -np.inf, np.inf, np.inf], [-np.inf, -150, np.inf], [-np.inf, np.nan, np.inf], [-150, np.nan, -50, np.nan, MINFLUX],
		[np.inf, np.inf, -150], [-np.inf, -150, -50, np.inf]]
	for n in list(range(1, 10)) + [1299, 1300]:
		for c in {0, n // 2 - 1, n // 2, n // 2 + 1, (n + 1) // 2, n} & set(range(n + 1)):
			cases.append([-150.0] * c + [-50.0] * (n - c))
			cases.append([-100.5] * c + [MINFLUX] * (n - c))
	return cases


def test_drop_pixel_equals_numpy_on_the_hand_cases(driver):
	cases = _hand_cases()
	got = drop_pixel(driver, cases)
	assert len(got) == len(cases)
	for x, g in zip(cases, got):
		assert g == numpy_rule(x), x


def test_drop_pixel_equals_numpy_on_random_series(driver):
	rng = np.random.default_rng(11)
	lengths = list(range(1, 10)) + [599, 600, 601, 1299, 1300]
	series = []
	for k in range(10000):
		n = lengths[k % len(lengths)] if k % 4 else int(rng.integers(1, 40))
		x = (MINFLUX + rng.normal(size=n) * rng.choice([0.01, 1.0, 50.0])).astype('float32')
		x[rng.random(n) < 0.05] = np.float32(MINFLUX)
		x[rng.random(n) < 0.03] = np.nan
		if k % 7 == 0:
			x[rng.random(n) < 0.2] = np.inf
		if k % 11 == 0:
			x[rng.random(n) < 0.2] = -np.inf
		series.append(x)
	got = drop_pixel(driver, series)
	assert len(got) == len(series)
	for k, x in enumerate(series):
		assert got[k] == numpy_rule(x), (k, x)


def test_finite_pixels_and_stamp_offsets(driver):
	x = np.array([0.0, -0.0, 1.0, np.finfo('float32').max, -np.finfo('float32').max, np.inf, -np.inf, np.nan, np.finfo('float32').smallest_subnormal], dtype='float32')
	g = (24, 120, 130, 200, 300, 6, 7, 2, 3)                       # n_frames, frame_rows, frame_cols, row0, col0, height, width, n_seg, n_targets
	st = (203, 209, 302, 309)
	p = np.arange(42)
	out = driver(f'finite {len(x)} ' + ' '.join(_hex32(x)) + '\noffset ' + ' '.join(map(str, g + st)) + f' {len(p)} ' + ' '.join(map(str, p)))
	assert [int(v) for v in out[0].split()] == np.isfinite(x).astype(int).tolist()
	assert [int(v) for v in out[1].split()] == ((st[0] - g[3] + p // g[6]) * g[2] + (st[2] - g[4] + p % g[6])).tolist()


# ---- (c) tables and argument checks -------------------------------------------------------------------------------------------------
def _solver(driver, offset, npix, ncad, history=10, status=None, align=4096, n=None):
	n = len(npix) if n is None else n
	status = [-1] * len(npix) if status is None else status
	text = f'solver {n} {len(npix)} {history} {align} ' + ' '.join(f'{o} {p} {c}' for o, p, c in zip(offset, npix, ncad)) + ' ' + ' '.join(map(str, status))
	return [line.split() for line in driver(text)]


def test_solver_layout_and_launch_lists(driver):
	rng = np.random.default_rng(41)
	shapes = [(1, 3), (4, 64), (5, 65), (63, 1), (64, 128), (65, 129), (484, 1300), (7, 0), (1257, 211)]
	probs = [halo.Problem(None, None, np.zeros((c, p), dtype='float32'), rng.random(c) < 0.9) for p, c in shapes]
	_, _, offset, npix, ncad = halo.pack(probs)
	history = 7
	status = [0, 1, 0, 4, 0, 2, 3, 0, 0]
	for st in (None, status):
		out = _solver(driver, offset, npix, ncad, history, st)
		assert out[0] == ['check', 'ok'] and out[1] == ['limit', 'ok']
		pitch, ntiles = (npix.astype('int64') + 3) // 4 * 4, (ncad.astype('int64') + 63) // 64
		first = lambda a: np.concatenate([[0], np.cumsum(a)[:-1]])
		want = np.stack([offset, first(ncad), first(pitch), first(npix), first(pitch) * history, first(ntiles * pitch), npix, pitch, ncad, ntiles], axis=1)
		got = np.array([[int(v) for v in w[1:]] for w in out[2:2 + len(shapes)]])
		assert np.array_equal(got, want)
		assert [int(v) for v in out[2 + len(shapes)][1:]] == [ncad.sum(), pitch.sum(), npix.sum(), (ntiles * pitch).sum(), ntiles.sum(), max(4, pitch.max())]
		active = [i for i in range(len(shapes)) if st is None or st[i] == 0]
		assert [int(v) for v in out[3 + len(shapes)][1:]] == active
		assert [int(v) for v in out[4 + len(shapes)][1:]] == [v for i in active for t in range(ntiles[i]) for v in (i, t)]


def test_solver_checks_reject_what_the_entries_reject(driver):
	ok = ([0, 16], [3, 4], [5, 6])
	assert _solver(driver, *ok)[0] == ['check', 'ok']
	assert ' '.join(_solver(driver, [], [], [], n=-1)[0][1:]) == 'tp_halo: bad problem count'
	assert ' '.join(_solver(driver, [], [], [], n=(1 << 24) + 1)[0][1:]) == 'tp_halo: bad problem count'
	assert _solver(driver, [], [], [], n=0) == [['check', 'ok']]
	assert ' '.join(_solver(driver, *ok, align=0)[0][1:]) == 'tp_halo: null pointer'
	assert ' '.join(_solver(driver, *ok, align=8)[0][1:]) == 'tp_halo: d_P must be 16-byte aligned'
	assert _solver(driver, *ok, align=32)[0] == ['check', 'ok']
	for npix in (0, 4097):
		assert ' '.join(_solver(driver, [0, 16], [3, npix], [5, 6])[0][1:]) == 'tp_halo: npix must lie in [1, 4096]'
	assert _solver(driver, [0, 16], [3, 4096], [5, 6])[0] == ['check', 'ok']
	assert ' '.join(_solver(driver, [0, 16], [3, 4], [5, -1])[0][1:]) == 'tp_halo: negative ncad'
	for off in (-4, 6):
		assert ' '.join(_solver(driver, [0, off], [3, 4], [5, 6])[0][1:]) == 'tp_halo: p_offset must be a non-negative multiple of 4'
	# 2^31 cadences in all
	assert ' '.join(_solver(driver, [0, 0], [1, 1], [2**30, 2**30])[1][1:]) == 'tp_halo: too many cadences'
	assert _solver(driver, [0, 0], [1, 1], [2**30, 2**30 - 1])[1] == ['limit', 'ok']
	h = lambda v: _hex64(v)[0]
	text = '\n'.join(f'settings {m} {H} {h(ft)} {h(gt)}' for m, H, ft, gt in ((101, 10, 2e-9, 1e-5), (0, 1, 0.0, 0.0), (5, 16, 0.0, 0.0), (-1, 10, 0.0, 0.0),
		(5, 0, 0.0, 0.0), (5, 17, 0.0, 0.0), (5, 10, -1e-9, 0.0), (5, 10, 0.0, -1e-9), (5, 10, np.nan, 0.0)))
	assert [int(line) for line in driver(text)] == [1, 1, 1, 0, 0, 0, 0, 0, 0]


def test_step_limit_and_poll_schedule(driver):
	out = driver('poll 0 101 7\npoll 0 0 3\npoll 1 0 3')
	assert [int(v) for v in out[0].split()] == [(101 + 1) * (hc.MAX_TRIALS + 1) + 1, 4, 8, 16, 32, 32, 32, 32]
	assert [int(v) for v in out[1].split()] == [hc.MAX_TRIALS + 2, 4, 8, 16]
	assert [int(v) for v in out[2].split()] == [1, 1, 2, 4]


@pytest.mark.parametrize('T', (1, 63, 64, 65, 1300))
def test_segment_lists(driver, T):
	rng = np.random.default_rng(T)
	n_seg = 3
	seg = rng.choice([-1, 0, 2], size=T, p=[0.1, 0.5, 0.4]) if T > 1 else np.array([2])         # segment 1 is empty
	seg[-1] = 2
	quality = rng.choice([0, 32, 16, 1 << 20], size=T)
	out = driver(f'seglists {T} {n_seg} {hc.DEFAULT_BITMASK} ' + ' '.join(f'{s} {q}' for s, q in zip(seg, quality)))
	got = {w[0]: [int(v) for v in w[1:]] for w in (line.split() for line in out)}
	cad = [np.flatnonzero(seg == k) for k in range(n_seg)]
	assert got['cadlist'] == np.concatenate(cad).tolist()
	assert got['fitlist'] == ((quality[np.concatenate(cad)] & hc.DEFAULT_BITMASK) == 0).astype(int).tolist()
	seg_off = np.concatenate([[0], np.cumsum([len(c) for c in cad])])
	assert got['seg_off'] == seg_off.tolist() and seg_off[1] == seg_off[2]
	tiles = [v for k in range(n_seg) for j in range(seg_off[k], seg_off[k + 1], 64) for v in (k, j, min(j + 64, seg_off[k + 1]))]
	assert got['tiles'] == tiles


GEOM = (24, 120, 130, 200, 300, 6, 7, 2, 3)                      # n_frames, frame_rows, frame_cols, row0, col0, height, width, n_seg, n_targets


def _stack(driver, g=GEOM, have_stack=1, stamps=None, seg=None):
	stamps = [[203, 209, 302, 309]] * g[8] if stamps is None else stamps
	seg = ([0] * 12 + [1] * 11 + [-1])[:max(g[0], 0)] if seg is None else seg
	words = list(g) + [have_stack, len(stamps)] + [v for s in stamps for v in s] + ([1] + list(seg) if seg != 'null' else [0])
	out = driver('stack ' + ' '.join(map(str, words)))
	return out[0].split(' ', 1)[1], out[1].split(' ', 1)[1]


def test_stack_and_segment_checks_reject_what_the_entries_reject(driver):
	assert _stack(driver) == ('ok', 'ok')
	edit = lambda k, v: GEOM[:k] + (v,) + GEOM[k + 1:]
	assert _stack(driver, have_stack=0)[0] == 'tp_halo: null pointer' and _stack(driver, stamps=[])[0] == 'tp_halo: null pointer'
	for k, v in ((0, 0), (1, 0), (2, 0), (8, 0), (8, 65536)):
		assert _stack(driver, g=edit(k, v), stamps=[[203, 209, 302, 309]])[0] == 'tp_halo: bad stack or batch size'
	for k, v in ((5, 0), (6, 0), (5, 4097)):
		assert _stack(driver, g=edit(k, v))[0] == 'tp_halo: a stamp holds 1 .. 4096 pixels'
	for v in (0, 65):
		assert _stack(driver, g=edit(7, v))[0] == 'tp_halo: 1 .. 64 segments'
	assert _stack(driver, stamps=[[203, 209, 302, 309], [203, 210, 302, 309], [203, 209, 302, 309]])[0] == "tp_halo: every stamp of a call has the call's height and width"
	for st in ([199, 205, 302, 309], [315, 321, 302, 309], [203, 209, 299, 306], [203, 209, 424, 431]):
		assert _stack(driver, stamps=[[203, 209, 302, 309], st, [203, 209, 302, 309]])[0] == 'tp_halo: stamp outside the frame stack'
	for st in ([200, 206, 300, 307], [314, 320, 423, 430]):                                       # the corners of the stack are inside
		assert _stack(driver, stamps=[st] * 3)[0] == 'ok'
	assert _stack(driver, seg='null')[1] == 'tp_halo: null pointer'
	assert _stack(driver, seg=[0] * 12 + [1] * 11 + [-2])[1] == 'tp_halo: segment below -1'
	for seg in ([0] * 24, [2] + [0] * 23, [-1] * 24):
		assert _stack(driver, seg=seg)[1] == 'tp_halo: n_seg must be the largest segment plus one'


def test_gather_and_norm_tables(driver):
	g = ' '.join(map(str, GEOM))
	index, npix, ncad = [0, 1, 4, 5], [42, 1, 7, 40], [12, 0, 24, 11]
	probs = [halo.Problem(None, None, np.zeros((c, p), dtype='float32'), np.ones(c, bool)) for p, c in zip(npix, ncad)]
	_, _, offset, _, _ = halo.pack(probs)
	out = driver(f'gather {g} 4 ' + ' '.join(f'{i} {o} {p} {c}' for i, o, p, c in zip(index, offset, npix, ncad)))
	assert out[0] == 'ok' and out[1] == 'max_ncad 24'
	c_off = np.concatenate([[0], np.cumsum(ncad)[:-1]])
	assert [[int(v) for v in line.split()[1:]] for line in out[2:]] == [[offset[r], c_off[r], index[r], npix[r], ncad[r], (npix[r] + 3) // 4 * 4] for r in range(4)]
	out = driver(f'norm {g} 4 ' + ' '.join(f'{i} {p} {c}' for i, p, c in zip(index, npix, ncad)))
	w_off = np.concatenate([[0], np.cumsum(npix)[:-1]])
	assert out[0] == 'ok'
	assert [[int(v) for v in line.split()[1:]] for line in out[1:5]] == [[c_off[r], w_off[r], index[r], npix[r], ncad[r]] for r in range(4)]
	assert [int(v) for v in out[5].split()[1:]] == [0, 1, -1, -1, 2, 3]
	assert driver(f'norm {g} 0') == ['ok', 'prob 0 0 0 0 0', 'run -1 -1 -1 -1 -1 -1']           # one entry for the upload, nothing run
	bad = lambda cmd, rows: driver(f'{cmd} {g} {len(rows)} ' + ' '.join(' '.join(map(str, r)) for r in rows))[0]
	for i in (-1, 6):
		assert bad('gather', [(i, 0, 1, 1)]) == 'tp_halo_gather_stack: problem index out of range'
		assert bad('norm', [(i, 1, 1)]) == 'tp_halo_outputs_stack: bad problem index'
	assert bad('norm', [(2, 1, 1), (2, 1, 1)]) == 'tp_halo_outputs_stack: bad problem index'  # a problem listed twice
	for p, c in ((0, 1), (43, 1), (1, -1), (1, 25)):
		assert bad('gather', [(0, 0, p, c)]) == 'tp_halo_gather_stack: npix or ncad out of range'
		assert bad('norm', [(0, p, c)]) == 'tp_halo_outputs_stack: npix or ncad out of range'
	for off in (-4, 2):
		assert bad('gather', [(0, off, 1, 1)]) == 'tp_halo_gather_stack: p_offset must be a non-negative multiple of 4'
	assert bad('gather', [(5, 0, 42, 24)]) == 'ok' and bad('norm', [(5, 42, 24)]) == 'ok'


# ---- (d) the state machine, composed ------------------------------------------------------------------------------------------------
def _lbfgs_text(P, fit, maxiter=hc.SETTINGS['maxiter'], history=hc.HISTORY):
	P = np.ascontiguousarray(P, dtype='float32')
	return (f'lbfgs {P.shape[1]} {P.shape[0]} {maxiter} {history} {_hex64(hc.FTOL)[0]} {_hex64(hc.GTOL)[0]} ' + ' '.join(map(str, np.asarray(fit, dtype=int)))
		+ ' ' + ' '.join(_hex32(P)))


def _lbfgs_parse(lines):
	out = []
	for head, w in zip(lines[0::2], lines[1::2]):
		status, iters, f = head.split()
		out.append({'status': int(status), 'iterations': int(iters), 'f': _f64(f), 'w': np.array([int(v, 16) for v in w.split()], dtype='uint64').view('float64')})
	return out


SHAPES = [(1, 3), (1, 130), (2, 3), (5, 10), (7, 64), (7, 65), (30, 211), (30, 212), (63, 129), (64, 128), (65, 193), (130, 300)]


def test_serial_optimiser_equals_the_restatement(driver):
	"""The whole optimiser run by the driver -- every transition and rule from the header, plain serial sums -- against
	``halo_common.lbfgs`` on 24 problems: status and iteration count equal, ``f`` within 1e-6 relative, and the weights within 1e-6
	except after a failed line search (where the last accepted point differs in the last digits and nothing pulls the two back)."""
	from test_gpu_halo import _problem
	probs = [_problem(npix, ncad, seed=base + i) for base in (2000, 3000) for i, (npix, ncad) in enumerate(SHAPES)]
	got = _lbfgs_parse(driver('\n'.join(_lbfgs_text(P, fit) for P, fit in probs)))
	assert len(got) == 24
	statuses, iterations = set(), []
	for k, ((P, fit), g) in enumerate(zip(probs, got)):
		ref = hc.lbfgs(P, fit)
		label = (SHAPES[k % 12], (2000, 3000)[k // 12] + k % 12)
		print(f"{label}: status {g['status']} / {ref['status']}, iterations {g['iterations']} / {ref['iterations']}, f {g['f']:.17g} / {ref['f']:.17g}, "
			f"max |dw| {np.max(np.abs(g['w'] - ref['w'])):.3e}")
		assert g['status'] == ref['status'], label
		assert g['iterations'] == ref['iterations'], label
		assert abs(g['f'] - ref['f']) <= 1e-6 * abs(ref['f']), label
		if ref['status'] != hc.LINESEARCH_FAILED:
			assert np.max(np.abs(g['w'] - ref['w'])) <= 1e-6, label
		statuses.add(ref['status'])
		iterations.append(ref['iterations'])
	assert statuses == {hc.CONVERGED, hc.CAP_REACHED, hc.LINESEARCH_FAILED} and min(iterations) == 0 and max(iterations) == 101


def test_degenerate_problems_no_iterations_and_short_histories(driver):
	from test_halo_host import _problem
	P, fit = _problem(5, 10, seed=4)
	fit[:] = False
	fit[:2] = True
	few, negative = (P, fit), (-np.abs(P), np.ones(10, bool))                                       # the two of test_degenerate_problems
	P, fit = _problem(30, 211, seed=211, n_dropped=10)
	runs = [(few, {}), (negative, {}), ((P, fit), {'maxiter': 0}), ((P, fit), {'history': 1}), ((P, fit), {'history': 16}), ((P, fit), {'maxiter': 3})]
	got = _lbfgs_parse(driver('\n'.join(_lbfgs_text(*p, **kw) for p, kw in runs)))
	for (p, kw), g in zip(runs, got):
		ref = hc.lbfgs(*p, **kw)
		assert (g['status'], g['iterations']) == (ref['status'], ref['iterations']), kw
		assert np.max(np.abs(g['w'] - ref['w'])) <= 1e-6
		assert (np.isnan(g['f']) and np.isnan(ref['f'])) or abs(g['f'] - ref['f']) <= 1e-6 * abs(ref['f'])
	assert [g['status'] for g in got[:3]] == [hc.DEGENERATE, hc.DEGENERATE, hc.CAP_REACHED] and got[2]['iterations'] == 0
	assert got[3]['iterations'] > 1 and got[4]['iterations'] > 16 and got[5]['status'] == hc.CAP_REACHED


FIELDS = ('status', 'iters', 'trials', 'need_grad', 'initial', 'n_pairs', 'newest')


def _machine(driver, events, nf=10, maxiter=101, history=10, ftol=hc.FTOL, gtol=hc.GTOL, objective=0):
	"""The states after init and after every scripted event: ``('s', ft, valid)`` or ``('f', gmax, sy, yy, gtd, gtd_steepest)``."""
	h = lambda v: _hex64(v)[0]
	words = [f'machine {nf} {maxiter} {history} {h(ftol)} {h(gtol)} {objective} {len(events)}']
	for e in events:
		words.append(f's {h(e[1])} {int(e[2])}' if e[0] == 's' else 'f ' + ' '.join(h(v) for v in e[1:]))
	out = []
	for line in driver('\n'.join(words)):
		w = line.split()
		st = dict(zip(FIELDS, map(int, w[1:8])))
		st.update(zip(('alpha', 'f', 'f_prev', 'gtd'), (_f64(v) for v in w[8:12])))
		st['slots'] = [int(v) for v in w[13:]]
		out.append(st)
	return out


def _pick(st, *names):
	return tuple(st[n] for n in names)


START = [('s', 10.0, True), ('f', 1.0, 0.0, 0.0, 0.0, -1.0)]          # the first point accepted, its gradient: steepest descent


def test_machine_first_point(driver):
	assert _pick(_machine(driver, [], nf=2)[0], 'status', 'initial', 'newest', 'alpha') == (hc.DEGENERATE, 1, -1, 1.0)      # fewer than 3 fitted cadences
	assert _machine(driver, [], nf=3)[0]['status'] == 0
	s = _machine(driver, [('s', 5.0, False)])                            # median <= 0 or not finite at the first point
	assert _pick(s[1], 'status', 'need_grad') == (hc.DEGENERATE, 0)
	s = _machine(driver, START)
	assert _pick(s[1], 'status', 'need_grad', 'initial', 'iters', 'f') == (0, 1, 1, 0, 10.0)
	assert _pick(s[2], 'status', 'need_grad', 'initial', 'n_pairs', 'newest', 'alpha', 'gtd', 'trials') == (0, 0, 0, 0, -1, 1.0, -1.0, 0)
	# |g|_inf <= gtol comes before the iteration cap; maxiter = 0 stops with status 2 and no iteration
	assert _pick(_machine(driver, [START[0], ('f', hc.GTOL, 0, 0, 0, -1.0)], maxiter=0)[2], 'status', 'iters', 'initial') == (hc.CONVERGED, 0, 0)
	assert _pick(_machine(driver, START, maxiter=0)[2], 'status', 'iters', 'initial', 'need_grad') == (hc.CAP_REACHED, 0, 0, 0)
	# tp_halo_objective: one evaluation
	assert _pick(_machine(driver, START, objective=1)[2], 'status', 'initial', 'need_grad') == (hc.CONVERGED, 0, 0)


def test_machine_line_search(driver):
	# f = 10, g.d = -1: a trial passes if ft <= 10 - 1e-4 alpha
	limit = 10.0 + hc.C1 * 1.0 * -1.0
	s = _machine(driver, START + [('s', np.nextafter(limit, 11.0), True), ('s', 1.0, False), ('s', 10.0 + hc.C1 * 0.25 * -1.0, True)])
	assert _pick(s[3], 'status', 'trials', 'alpha', 'need_grad', 'iters') == (0, 1, 0.5, 0, 0)
	assert _pick(s[4], 'status', 'trials', 'alpha', 'need_grad', 'iters') == (0, 2, 0.25, 0, 0)          # an invalid trial fails whatever its f
	assert _pick(s[5], 'status', 'trials', 'alpha', 'need_grad', 'iters', 'f', 'f_prev') == (0, 2, 0.25, 1, 1, 10.0 + hc.C1 * 0.25 * -1.0, 10.0)
	assert _pick(_machine(driver, START + [('s', limit, True)])[3], 'need_grad', 'iters', 'alpha') == (1, 1, 1.0)
	# twenty trials that fail: status 3, theta kept (no iteration), alpha stays at the last trial's
	s = _machine(driver, START + [('s', 11.0, True)] * hc.MAX_TRIALS)
	assert [st['trials'] for st in s[3:]] == list(range(1, hc.MAX_TRIALS + 1))
	assert [st['status'] for st in s[3:]] == [0] * (hc.MAX_TRIALS - 1) + [hc.LINESEARCH_FAILED]
	assert _pick(s[-1], 'alpha', 'iters', 'need_grad', 'f') == (0.5**(hc.MAX_TRIALS - 1), 0, 0, 10.0)


def _steps(n, sy=1.0, yy=1.0, gtd=-2.0):
	"""``n`` accepted iterations: f falls by 0.1 each, the pair (sy, yy), the two-loop direction with g.d = gtd."""
	ev = []
	for i in range(1, n + 1):
		ev += [('s', 10.0 - 0.1 * i, True), ('f', 1.0, sy, yy, gtd, -1.0)]
	return ev


@pytest.mark.parametrize('history', (1, 10, 16))
def test_machine_history_ring(driver, history):
	s = _machine(driver, START + _steps(20), history=history)[3:][1::2]            # the states after every finish
	for i, st in enumerate(s, start=1):
		n_pairs, newest = min(i, history), (i - 1) % history
		assert _pick(st, 'status', 'iters', 'n_pairs', 'newest', 'gtd', 'alpha', 'trials') == (0, i, n_pairs, newest, -2.0, 1.0, 0)
		assert st['slots'] == [(newest - (n_pairs - 1 - j)) % history for j in range(n_pairs)]      # oldest .. newest
	if history == 16:
		assert s[-1]['slots'] == list(range(4, 16)) + [0, 1, 2, 3]


def test_machine_rejected_pair_and_dropped_history(driver):
	keep, reject = np.nextafter(hc.PAIR_CURV * 3.0, 1.0), hc.PAIR_CURV * 3.0
	ev = START + _steps(3) + [('s', 9.6, True), ('f', 1.0, reject, 3.0, -2.0, -1.0), ('s', 9.5, True), ('f', 1.0, keep, 3.0, -2.0, -1.0)]
	s = _machine(driver, ev)
	assert _pick(s[-3], 'iters', 'n_pairs', 'newest') == (4, 3, 2) and s[-3]['slots'] == [0, 1, 2]     # s.y <= 1e-10 y.y: not stored
	assert _pick(s[-1], 'iters', 'n_pairs', 'newest') == (5, 4, 3)
	# not a descent direction (g.d >= 0, or NaN): the history is dropped, steepest descent; the next pair goes to the next slot
	for gtd in (0.0, 0.5, np.nan):
		s = _machine(driver, START + _steps(3) + [('s', 9.6, True), ('f', 1.0, 1.0, 1.0, gtd, -0.75)] + [('s', 9.5, True), ('f', 1.0, 1.0, 1.0, -2.0, -1.0)])
		assert _pick(s[-3], 'status', 'iters', 'n_pairs', 'newest', 'gtd') == (0, 4, 0, 3, -0.75) and s[-3]['slots'] == []
	assert _pick(s[-1], 'n_pairs', 'newest', 'gtd') == (1, 4, -2.0) and s[-1]['slots'] == [4]


def test_machine_stopping_tests_in_their_order(driver):
	small = 10.0 - hc.FTOL * 10.0                                                     # f_k - f_k+1 = ftol max(|f_k|, |f_k+1|, 1), to rounding
	tail = lambda ft, gmax, **kw: _machine(driver, START[:1] + [('f', 1.0, 0, 0, 0, -1e-9), ('s', ft, True), ('f', gmax, 1.0, 1.0, -2.0, -1.0)], **kw)[-1]
	assert _pick(tail(np.nextafter(small, 11.0), 1.0), 'status', 'iters', 'n_pairs', 'newest', 'initial') == (hc.CONVERGED, 1, 1, 0, 0)
	assert _pick(tail(9.0, hc.GTOL), 'status', 'iters') == (hc.CONVERGED, 1)
	assert _pick(tail(9.0, 1.0, maxiter=1), 'status', 'iters') == (hc.CAP_REACHED, 1)
	assert _pick(tail(9.0, hc.GTOL, maxiter=1), 'status', 'iters') == (hc.CONVERGED, 1)          # converged comes before the cap
	assert _pick(tail(9.0, 1.0, maxiter=2), 'status', 'iters', 'gtd') == (0, 1, -2.0)
	# a stopped problem takes no further step
	s = _machine(driver, START + [('s', 9.0, True), ('f', hc.GTOL, 1.0, 1.0, -2.0, -1.0), ('s', 8.0, True), ('f', 1.0, 1.0, 1.0, -2.0, -1.0)])
	assert s[-1] == s[-3]
