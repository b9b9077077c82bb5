# -*- coding: utf-8 -*-
"""
The case table of tests/test_gpu_cutout_paths.py (tests/cutout_common.py) held, without a GPU, to what it claims: every case takes the
path its name says with the stamps it really gets, the table as a whole reaches every class of the stamp cutter's launch code
(csrc/cutout.hip, ``cut_stamps_launch``), the restated rules agree with ``layout_common.cut_path`` and with the comment of
test_gpu_cutout.py, and the stamps and expectations are what the GPU tests take them for.
"""
import numpy as np
import pytest
import cutout_common as cc
import layout_common as lc


@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_every_case_takes_the_path_of_its_name(name):
	c = cc.CASES[name]
	stamps = cc.case_stamps(name)
	assert len(stamps) == c['n'] + cc.N_EXTRA
	want = {'g': 'gather', 't': 'tiles'}[name.split('_')[0]]
	facts = cc.launch_facts(c['T'], c['R'], c['C'], c['H'], c['W'], len(stamps), t_pitch=c['t_pitch'])
	assert facts == cc.case_facts(name)
	assert facts['path'] == want
	masked = cc.launch_facts(c['T'], c['R'], c['C'], c['H'], c['W'], len(stamps), t_pitch=c['t_pitch'], masked=True)
	assert masked['path'] == {'gather': 'gather', 'tiles': 'tiles_pixels'}[want]
	assert not facts['refused']
	assert np.all(stamps[:, 1] - stamps[:, 0] == c['H']) and np.all(stamps[:, 3] - stamps[:, 2] == c['W'])


def test_the_table_reaches_every_class():
	gather = {k: cc.case_facts(k) for k in cc.CASES if k.startswith('g_')}
	tiles = {k: cc.case_facts(k) for k in cc.CASES if k.startswith('t_')}
	assert {1, 2, 3, 4, 5, 7, 16, 40} <= {f['wgrp'] for f in gather.values()}
	# every segment walk that carries (16 % wgrp != 0) also with a block of 64 real cadences: each LDS slot of the tile is stored
	assert {3, 5, 7} <= {f['wgrp'] for k, f in gather.items() if cc.CASES[k]['T'] >= 64}
	assert {1, 2, 3, 4} <= {f['band_rows'] for f in gather.values()}
	assert any(f['last_band_rows'] < f['band_rows'] for f in gather.values())
	assert any(f['band_rows'] == 1 and f['n_bands'] > 1 for f in gather.values())         # bands of one row: di = 0
	assert {True, False} <= {f['needs_attribute'] for f in gather.values()}
	assert {1, 2, 3} <= {f['scan_per'] for f in tiles.values()}
	assert any(f['cad_blocks_beyond'] > 0 and f['cad_block'] == 64 for f in gather.values())
	assert any(f['cad_blocks_beyond'] > 0 and f['cad_block'] == 32 for f in tiles.values())
	# what the rows are there for, one by one
	f = gather['g_62x17']
	assert (f['wgrp'], f['band_rows'], f['last_band_rows']) == (2, 3, 2)
	f = gather['g_5x32']
	assert (f['wgrp'], f['band_rows'], f['last_band_rows']) == (2, 2, 1)
	assert (gather['g_4x33']['wgrp'], gather['g_4x33']['band_rows']) == (3, 1)
	assert (gather['g_3x64']['wgrp'], gather['g_3x64']['band_rows']) == (4, 1)
	assert (gather['g_2x65']['wgrp'], gather['g_2x65']['band_rows']) == (5, 1)
	assert gather['g_3x100']['wgrp'] == 7
	assert (gather['g_45x67']['wgrp'], gather['g_45x67']['cad_blocks']) == (3, 2) and gather['g_45x67']['cad_blocks_beyond'] == 0
	assert gather['g_2x256']['shmem'] == 65792 and gather['g_2x256']['needs_attribute']
	assert gather['g_1x639']['shmem'] == 163584 and cc.CASES['g_1x639']['W'] > cc.CASES['g_1x639']['C']
	assert gather['g_pitch_odd']['t_pitch'] % 4 != 0
	assert gather['g_pitch_far']['cad_blocks_beyond'] >= 2
	assert tiles['t_scan_1024']['n_tiles'] == 1024 and tiles['t_scan_1024']['scan_per'] == 1
	assert tiles['t_scan_1040']['n_tiles'] == 1040 and tiles['t_scan_1040']['scan_per'] == 2
	assert tiles['t_scan_2210']['n_tiles'] == 17 * 130 and tiles['t_scan_2210']['scan_per'] == 3 and cc.CASES['t_scan_2210']['C'] % 64 == 6
	assert tiles['t_pitch_odd']['t_pitch'] % 4 != 0
	assert tiles['t_pitch_far']['cad_blocks_beyond'] >= 2
	assert cc.CASES['t_9x70']['R'] % 2 == 1 and cc.CASES['t_9x70']['C'] % 64 != 0
	assert cc.CASES['t_1cad']['T'] == 1
	assert all(v != 0 for v in cc.CASES['t_offsets']['offsets']) and all(v != 0 for v in cc.CASES['g_offsets']['offsets'])


def test_the_table_stays_small():
	"""Frame stacks and cubes of a few megabytes.  The two gather cases with large stamps are the exception: their 14 stamps must cover
	less than an eighth of the frame, and the cadence count (a second 64-block) is what g_45x67 is there for."""
	for name, c in cc.CASES.items():
		f = cc.case_facts(name)
		stack = c['T'] * c['R'] * c['C'] * 4
		cube = (c['n'] + cc.N_EXTRA) * c['H'] * c['W'] * f['t_pitch'] * 4
		assert stack < (100 << 20 if name == 'g_45x67' else 20 << 20), name
		assert cube < (17 << 20 if name == 'g_45x67' else 5 << 20), name


def test_rules_agree_with_layout_common():
	for (T, R, C, H, W, n) in lc.CUT_CASES:
		for count in (n, n + 8):            # as the table has them, and with the 8 edge stamps cut_stamps adds
			assert cc.launch_facts(T, R, C, H, W, count)['path'] == lc.cut_path(R, C, H, W, count)
	assert [lc.cut_path(R, C, H, W, n + 8) for (T, R, C, H, W, n) in lc.CUT_CASES] == ['tiles', 'gather']


def test_rules_agree_with_the_comment_of_test_gpu_cutout():
	"""test_gpu_cutout.py::test_against_oracle: "the first four and the sixth case take the tile-major path, the fifth and the last the
	per-stamp gather"."""
	shapes = [(64, 30, 30, 15, 15, 25), (129, 50, 70, 11, 17, 25), (200, 64, 64, 21, 16, 25), (7, 20, 20, 5, 3, 25),
		(70, 200, 300, 15, 15, 5), (131, 97, 203, 15, 15, 400), (65, 31, 400, 9, 70, 2)]
	paths = [cc.launch_facts(*s)['path'] for s in shapes]
	assert paths == ['tiles', 'tiles', 'tiles', 'tiles', 'gather', 'tiles', 'gather']


def test_the_width_limit():
	assert not cc.launch_facts(33, 200, 300, 1, 639, 1)['refused']
	assert cc.launch_facts(33, 200, 300, 1, 640, 1)['refused']
	assert cc.launch_facts(33, 200, 300, 1, 639, 1)['shmem'] <= cc.LDS_LIMIT < cc.launch_facts(33, 200, 300, 1, 640, 1)['shmem']
	assert not cc.launch_facts(33, 200, 300, 2, 255, 1)['needs_attribute'] and cc.launch_facts(33, 200, 300, 2, 256, 1)['needs_attribute']


@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_stamps_and_expectation(name):
	"""The four outside stamps miss the frame (all NaN), the left one ends exactly at column 0, the last stamp is stamp 0 again, the
	edge stamps hold both NaN and pixels."""
	c = cc.CASES[name]
	R, C, H, W = c['R'], c['C'], c['H'], c['W']
	ro, co = c['offsets']
	frames = np.arange(2 * R * C, dtype='float32').reshape(2, R, C) + 1      # finite everywhere: a NaN in the cube is a pixel off the frame
	stamps = cc.case_stamps(name)
	want = cc.expected(frames, stamps, ro, co)
	assert want.shape == (len(stamps), H, W, 2) and want.dtype == np.float32
	assert np.all(np.isnan(want[cc.OUTSIDE]))
	left = stamps[cc.OUTSIDE][2]
	assert left[3] - co == 0
	np.testing.assert_array_equal(stamps[cc.DUPLICATE], stamps[0])
	np.testing.assert_array_equal(want[cc.DUPLICATE], want[0])
	if H >= 3 and W >= 3:      # (a stamp of one or two rows that sticks out by two is outside)
		for w in want[cc.EDGE]:
			assert np.any(np.isnan(w)) and not np.all(np.isnan(w))
	assert np.any(~np.isnan(want[:c['n']]))


def test_the_oracle_slices_like_numpy():
	T, R, C, H, W = 3, 20, 30, 5, 7
	frames = cc.make_frames(T, R, C, seed=1)
	for (r1, c1, ro, co) in ((0, 0, 0, 0), (4, 9, 0, 44), (R - H, C - W, 100, 44)):
		stamp = (r1 + ro, r1 + H + ro, c1 + co, c1 + W + co)
		want = np.moveaxis(frames[:, r1:r1 + H, c1:c1 + W], 0, 2)
		got = cc.expected(frames, [stamp], ro, co)[0]
		assert got.shape == (H, W, T)
		np.testing.assert_array_equal(got.view('uint32'), np.ascontiguousarray(want).view('uint32'))


def test_frames_hold_the_values_arithmetic_destroys():
	f = cc.make_frames(5, 30, 30, seed=2)
	assert f.dtype == np.float32 and f.shape == (5, 30, 30)
	assert np.any(np.isnan(f)) and np.any(f == np.inf) and np.any(f == -np.inf)
	assert np.any((f == 0) & np.signbit(f))
	assert 0.005 < np.mean(np.isnan(f)) < 0.05
