# -*- coding: utf-8 -*-
"""
The host-side rules of a batched run over target pixel files (``tessphot_tpfs``), none of which needs a device: where
``tpf.load_tpf_groups`` puts every file (``tpf.bucket_files`` / ``tpf.plan_groups``: a pure function of the header shapes and the kept
rows), which star is a file's main target (``tpf.main_targets``), how many files make a chunk (``tessphot.tpf_chunk_files``) and what
the plugin makes of the device flags of the one attempt a ``tpf`` stamp gets (``tessphot._one_attempt``).  The expected values are
worked out by hand in the comments.
"""
import numpy as np
import pytest
from photometry_amd import tpf
from photometry_amd.tessphot import tpf_chunk_files, _one_attempt, TPF_CHUNK_SHARE
from photometry_amd.status import STATUS

A, B, C = (11, 11, 70), (7, 9, 70), (1, 1, 33)


def _replay(shapes, kept):
	"""Carry the plan out on lists standing in for the cubes: ``[group][slot]`` -> file, every move reading a slot that holds a file."""
	keys, members = tpf.bucket_files(shapes)
	groups, index, moves = tpf.plan_groups(shapes, kept)
	bucket = [list(m) for m in members]
	cubes = [bucket[b] if not own else [None] * len(files) for (_, b, own, files) in groups]
	for b, src, g, slot in moves:
		assert bucket[b][src] is not None, (b, src)
		cubes[g][slot], bucket[b][src] = bucket[b][src], None
	for g, (shape, b, own, files) in enumerate(groups):
		assert cubes[g][:len(files)] == files, (g, cubes[g], files)
		assert all(shapes[i][:2] == shape[:2] and kept[i] == shape[2] for i in files)
		if not own:
			assert all(v is None for v in cubes[g][len(files):])           # nothing is left behind the regular files
	assert sorted(i for (_, _, _, files) in groups for i in files) == list(range(len(shapes)))
	for i, (g, slot) in enumerate(index):
		assert groups[g][3][slot] == i
	return groups, index, moves


def test_buckets_are_header_shapes_in_order_of_appearance():
	keys, members = tpf.bucket_files([A, B, A, C, B, A])
	assert keys == [A, B, C] and members == [[0, 2, 5], [1, 4], [3]]


def test_all_equal_moves_nothing():
	groups, index, moves = _replay([A, A, A], [70, 70, 70])
	assert groups == [((11, 11, 70), 0, False, [0, 1, 2])] and index == [(0, 0), (0, 1), (0, 2)] and moves == []


def test_odd_one_first_leaves_a_hole_that_the_last_regular_file_fills():
	# slots 0..3 hold files 0..3; file 0 (68 rows kept) goes to its own group, slot 0 is then filled from slot 3
	groups, index, moves = _replay([A] * 4, [68, 70, 70, 70])
	assert groups == [((11, 11, 70), 0, False, [3, 1, 2]), ((11, 11, 68), 0, True, [0])]
	assert index == [(1, 0), (0, 1), (0, 2), (0, 0)]
	assert moves == [(0, 0, 1, 0), (0, 3, 0, 0)]


def test_odd_one_last_costs_one_move():
	groups, index, moves = _replay([A] * 4, [70, 70, 70, 68])
	assert groups == [((11, 11, 70), 0, False, [0, 1, 2]), ((11, 11, 68), 0, True, [3])]
	assert index == [(0, 0), (0, 1), (0, 2), (1, 0)] and moves == [(0, 3, 1, 0)]


def test_two_odd_ones_with_the_same_T_share_a_group():
	# files 1 and 3 leave; three regular files want slots 0..2: slot 1 is filled from slot 4, the hole at slot 3 lies behind them
	groups, index, moves = _replay([A] * 5, [70, 68, 70, 68, 70])
	assert groups == [((11, 11, 70), 0, False, [0, 4, 2]), ((11, 11, 68), 0, True, [1, 3])]
	assert index == [(0, 0), (1, 0), (0, 2), (1, 1), (0, 1)]
	assert moves == [(0, 1, 1, 0), (0, 3, 1, 1), (0, 4, 0, 1)]


def test_two_odd_ones_with_different_T_get_a_group_each():
	groups, index, moves = _replay([A] * 5, [69, 70, 68, 70, 70])
	assert [g[0] for g in groups] == [(11, 11, 70), (11, 11, 69), (11, 11, 68)]
	assert groups[0][3] == [4, 1, 3] and groups[1][3] == [0] and groups[2][3] == [2]
	assert moves == [(0, 0, 1, 0), (0, 2, 2, 0), (0, 4, 0, 0), (0, 3, 0, 2)]


def test_a_bucket_of_one_and_dropped_rows_that_are_the_rule():
	groups, index, moves = _replay([C], [33])
	assert groups == [((1, 1, 33), 0, False, [0])] and moves == []
	groups, index, moves = _replay([C], [30])                                # the only file dropped rows: its T is the bucket's
	assert groups == [((1, 1, 30), 0, False, [0])] and moves == []
	groups, index, moves = _replay([A] * 3, [68, 68, 68])                    # a sector's files usually miss the same rows
	assert groups == [((11, 11, 68), 0, False, [0, 1, 2])] and moves == []


def test_a_tie_goes_to_the_T_met_first_and_buckets_do_not_mix():
	groups, index, moves = _replay([A, B, A, B], [70, 40, 70, 39])
	assert groups == [((11, 11, 70), 0, False, [0, 2]), ((7, 9, 40), 1, False, [1]), ((7, 9, 39), 1, True, [3])]
	assert index == [(0, 0), (1, 0), (0, 1), (2, 0)] and moves == [(1, 1, 2, 0)]


@pytest.mark.parametrize('seed', range(20))
def test_random_plans_replay(seed):
	rng = np.random.default_rng(seed)
	n = int(rng.integers(1, 25))
	shapes = [(A, B, C)[k] for k in rng.integers(0, 3, n)]
	kept = [int(s[2] - rng.choice([0, 0, 0, 1, 2])) for s in shapes]
	groups, index, moves = _replay(shapes, kept)
	odd = sum(len(files) for (_, _, own, files) in groups if own)
	assert len(moves) <= 2 * odd                                             # one move out, at most one into the hole


# ---- main targets ----------------------------------------------------------------------------------------------------------------
def test_main_target_is_the_ticid_unless_targets_names_the_file():
	files = ['/d/a_tp.fits', '/d/b_tp.fits', '/d/c_tp.fits']
	assert tpf.main_targets(files, [11, 22, 33]) == [11, 22, 33]
	targets = {'starid': np.array([5, 6, 7]), 'tmag': np.zeros(3), 'row': np.zeros(3), 'column': np.zeros(3)}
	assert tpf.main_targets(files, [11, 22, 33], targets) == [11, 22, 33]     # no 'file' column: targets only place the stars
	targets['file'] = [None, '/d/b_tp.fits', '']
	assert tpf.main_targets(files, [11, 22, 33], targets) == [11, 6, 33]


def test_a_file_listed_once_per_extra_target():
	files = ['/d/a_tp.fits', '/d/b_tp.fits', '/d/a_tp.fits']
	targets = {'starid': np.array([11, 99, 22]), 'file': ['/d/a_tp.fits', '/d/a_tp.fits', None]}
	assert tpf.main_targets(files, [11, 22, 11], targets) == [11, 22, 99]
	with pytest.raises(ValueError, match=r'/d/a_tp\.fits: listed 3 times'):
		tpf.main_targets(files + ['/d/a_tp.fits'], [11, 22, 11, 11], targets)
	with pytest.raises(ValueError, match='no TICID'):
		tpf.main_targets(['/d/x_tp.fits'], [None])


# ---- chunks ----------------------------------------------------------------------------------------------------------------------
def test_chunk_size_rule():
	assert TPF_CHUNK_SHARE == 0.25
	# 11 x 11 x 19 000: 19 008 cadences of pitch, 3 cubes of 121 series of 4-byte values = 27 599 616 bytes a file
	per_file = 3 * 4 * 121 * 19008
	assert per_file == 27599616
	shapes = [(11, 11, 19000)] * 5000
	assert tpf_chunk_files(shapes, 4 * 100 * per_file) == 100                 # a quarter of the free memory
	assert tpf_chunk_files(shapes, 4 * 100 * per_file - 4) == 99
	assert tpf_chunk_files(shapes, 1 << 40) == 4096                           # the cap
	assert tpf_chunk_files(shapes[:7], 1 << 40) == 7                          # never more than there are
	assert tpf_chunk_files(shapes, 1000) == 1                                 # at least one
	assert tpf_chunk_files([(1, 1, 33), (11, 11, 19000)], 4 * 2 * per_file) == 2   # sized by the largest file
	assert tpf_chunk_files(shapes, 8 * 10 * per_file, share=0.125) == 10


# ---- the plugin's reading of one attempt -------------------------------------------------------------------------------------------
def test_one_attempt_in_the_plugins_words():
	assert _one_attempt(0) == (STATUS.OK, True, [])
	assert _one_attempt(4) == (STATUS.OK, True, ['WARNING: Could not resize stamp any further.'])
	assert _one_attempt(1) == (STATUS.WARNING, True, ['WARNING: No mask found for main target. Using minimum aperture.'])
	assert _one_attempt(1 | 32) == (STATUS.WARNING, True, ['ERROR: No flux above threshold.', 'WARNING: No masks found. Using minimum aperture.'])
	assert _one_attempt(5 << 8) == (STATUS.ERROR, False, ['ERROR: Too many masks.'])
	assert _one_attempt(6 << 8) == (STATUS.ERROR, True, ['ERROR: No targets in mask.'])
	assert _one_attempt(1 << 8) == (STATUS.ERROR, False, ['RuntimeError: K2P2NoFlux: No measured flux in sum-image'])
