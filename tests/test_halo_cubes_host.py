# -*- coding: utf-8 -*-
"""
CPU check of the cubes path's device-free rules (photometry_amd/csrc/halo_rules.h: ``CubeGeom`` and its checks, ``cube_lists``, the
per-target problem indexing, the gather / outputs tables): the header compiled for the host with AddressSanitizer and UBSan into the
stand-alone driver tests/hostsim/halo_cubes_host.cpp, which composes them serially, and held to numpy and to ``photometry_amd.halo``.
"""
import os
import subprocess
import numpy as np
import pytest
import conftest
from photometry_amd import halo

SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'halo_cubes_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'halo_cubes_host')


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


def _lists(driver, geom, prob_off, seg, quality, bitmask=175, have_cube=1):
	n, H, W, T, pitch = geom
	cells = ' '.join(f'{s} {q}' for s, q in zip(np.asarray(seg).ravel(), np.asarray(quality).ravel()))
	return driver(f"lists {n} {H} {W} {T} {pitch} {bitmask} {have_cube} {' '.join(map(str, prob_off))} {cells}")


def _ints(line, skip=1):
	return [int(v) for v in line.split()[skip:]]


def test_lists_and_problem_indexing_equal_numpy(driver):
	rng = np.random.default_rng(3)
	for n_seg in ([1], [3, 1, 2], [2, 64, 1], [1, 1, 1, 5]):
		n, T, bitmask = len(n_seg), int(rng.integers(1, 90)), 175
		seg = np.stack([rng.integers(-1, k, size=T) for k in n_seg])
		if n > 1:
			seg[1][seg[1] == 0] = -1                                         # segment 0 of target 1 has no cadence
		quality = np.where(rng.random((n, T)) < 0.3, 1 << rng.integers(0, 13, size=(n, T)), 0)
		off = np.concatenate([[0], np.cumsum(n_seg)])
		out = _lists(driver, (n, 3, 4, T, T + 5), off, seg, quality, bitmask)
		assert out[0] == 'cube ok' and out[1] == 'seg ok' and out[2] == f'n_prob {off[-1]}'
		assert _ints(out[3]) == list(np.repeat(np.arange(n), n_seg))
		lo, hi = _ints(out[4]), _ints(out[5])
		rows = out[6:6 + 2 * n]
		serial = out[6 + 2 * n:6 + 2 * n + off[-1]]
		for i in range(n):
			cadlist, fitlist = _ints(rows[2 * i], 2), _ints(rows[2 * i + 1], 2)
			order = [t for k in range(n_seg[i]) for t in np.flatnonzero(seg[i] == k)]
			assert cadlist[:len(order)] == order and len(cadlist) == T
			assert fitlist[:len(order)] == [int((quality[i][t] & bitmask) == 0) for t in order]
			for k in range(n_seg[i]):
				q = off[i] + k
				want = list(np.flatnonzero(seg[i] == k))
				assert hi[q] - lo[q] == len(want) and _ints(serial[q], 2) == want
				assert lo[q] == (0 if k == 0 else hi[q - 1])
			# the same cadences and fit flags as the host restatement's problems see
			c_all = [np.flatnonzero(seg[i] == k) for k in range(n_seg[i])]
			assert [len(c) for c in c_all] == [hi[off[i] + k] - lo[off[i] + k] for k in range(n_seg[i])]
		HW, pitch = 12, T + 5
		assert _ints(out[-1]) == [0, (HW - 1) * pitch, (n - 1) * HW * pitch, ((n - 1) * HW + HW - 1) * pitch]
	# the segments halo.segments makes go through as they are
	time = 1500.0 + np.arange(40) * 0.03
	time[20:] += 0.51
	seg = halo.segments(time, halo.split_times(-1, time, np.zeros(40)))
	out = _lists(driver, (1, 2, 2, 40, 64), [0, 2], seg[None], np.zeros((1, 40), dtype=int))
	assert out[1] == 'seg ok' and _ints(out[4]) == [0, 20] and _ints(out[5]) == [20, 40]


def test_checks_reject_what_the_entries_reject(driver):
	seg, q = np.zeros((2, 4), dtype=int), np.zeros((2, 4), dtype=int)
	ok = lambda **kw: _lists(driver, kw.pop('geom', (2, 4, 5, 4, 32)), kw.pop('off', [0, 1, 2]), kw.pop('seg', seg), q, **kw)
	assert ok()[:2] == ['cube ok', 'seg ok']
	assert ok(have_cube=0)[0] == 'cube tp_halo: null pointer'
	assert ok(geom=(2, 65, 64, 4, 32))[0] == 'cube tp_halo: a stamp holds 1 .. 4096 pixels'
	assert ok(geom=(2, 64, 64, 4, 32))[0] == 'cube ok'
	assert ok(geom=(2, 0, 5, 4, 32))[0] == 'cube tp_halo: a stamp holds 1 .. 4096 pixels'
	assert ok(geom=(2, 4, 5, 4, 3))[0] == 'cube tp_halo: bad cube or batch size'                  # t_pitch < n_cad
	assert ok(off=[0, 65, 66])[0] == 'cube tp_halo: h_prob_off must rise by 1 .. 64 segments per target'
	assert ok(off=[0, 64, 65], seg=np.full((2, 4), 0))[:2] == ['cube ok', 'seg ok']
	assert ok(off=[0, 2, 1])[0] == 'cube tp_halo: h_prob_off must rise by 1 .. 64 segments per target'   # not monotone
	assert ok(off=[0, 1, 1])[0] == 'cube tp_halo: h_prob_off must rise by 1 .. 64 segments per target'   # a target without a segment
	assert ok(off=[1, 2, 3])[0] == 'cube tp_halo: h_prob_off must start at 0'
	for value in (1, -2):
		bad = seg.copy()
		bad[1, 3] = value
		assert ok(seg=bad)[1] == 'seg tp_halo: segment outside -1 .. n_seg - 1 of its target'
	bad = seg.copy()
	bad[0, 0] = 2
	assert ok(off=[0, 3, 4], seg=bad)[1] == 'seg ok' and ok(off=[0, 2, 5], seg=bad)[1].startswith('seg tp_halo: segment outside')


def test_gather_and_norm_tables(driver):
	geom, off = (3, 4, 5, 30, 32), [0, 2, 3, 6]
	index, npix, ncad = [0, 1, 3, 4, 5], [20, 1, 7, 13, 4], [12, 0, 30, 11, 2]
	probs = [halo.Problem(None, None, np.zeros((c, p), dtype='float32'), np.ones(c, bool)) for p, c in zip(npix, ncad)]
	_, _, p_off, _, _ = halo.pack(probs)
	run = lambda index=index, p_off=p_off, npix=npix, ncad=ncad: driver(f"tables {' '.join(map(str, geom))} {' '.join(map(str, off))} {len(index)} " +
		' '.join(f'{i} {o} {p} {c}' for i, o, p, c in zip(index, p_off, npix, ncad)))
	out = run()
	assert out[0] == 'gather ok' and out[1] == f'sizes {max(ncad)} {(max(npix) + 3) // 4 * 4}'
	c_off = np.concatenate([[0], np.cumsum(ncad)])
	w_off = np.concatenate([[0], np.cumsum(npix)])
	for r in range(len(index)):
		assert _ints(out[2 + r], 0) == [p_off[r], c_off[r], index[r], npix[r], ncad[r], (npix[r] + 3) // 4 * 4]
	k = 2 + len(index)
	assert out[k] == 'norm ok'
	for r in range(len(index)):
		assert _ints(out[k + 1 + r], 0) == [c_off[r], w_off[r], index[r], npix[r], ncad[r]]
	assert _ints(out[k + 1 + len(index)]) == [0, 1, -1, 2, 3, 4]
	assert run(index=[0, 1, 3, 4, 6])[0].startswith('gather tp_halo_gather_cubes:')                    # past the last problem
	assert run(npix=[21, 1, 7, 13, 4])[0].startswith('gather tp_halo_gather_cubes:')                   # more pixels than the stamp
	assert run(ncad=[12, 0, 31, 11, 2])[0].startswith('gather tp_halo_gather_cubes:')                  # more cadences than the cube
	assert run(p_off=[0, 242, 240, 480, 656])[0].startswith('gather tp_halo_gather_cubes:')            # not a multiple of 4
	assert any(line.startswith('norm tp_halo_outputs_cubes:') for line in run(index=[0, 1, 3, 3, 5]))   # a problem twice
