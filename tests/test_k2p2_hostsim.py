# -*- coding: utf-8 -*-
"""
CPU check of the K2P2 KERNEL LOGIC: photometry_amd/csrc/k2p2_core.h compiled for the host
(lane layer tests/hostsim/k2p2_lanes_host.h: lanes become loops; test-only, see tests/hostsim/k2p2_hostsim.cpp) against the
oracle.  The real parity test of the HIP kernel is tests/test_gpu_k2p2.py.
"""
import numpy as np
import pytest
from k2p2_common import make_cases, oracle_batch, compare, build_hostsim, run_hostsim


@pytest.fixture(scope='module')
def hostsim():
	return build_hostsim()


@pytest.mark.parametrize("kind,seed", [('faint15', 1), ('small11', 2), ('crowded', 3), ('bright', 4), ('tiny', 5), ('faint15', 6), ('wide', 7), ('wide', 8), ('huge', 6)])
def test_hostsim_matches_oracle(hostsim, kind, seed):
	s, S = make_cases(kind, seed)
	got = run_hostsim(hostsim, s, S)
	ref = oracle_batch(s, S)
	stats = compare(s, S, got, ref)
	print(kind, stats)
	assert stats['n_exact'] + stats['n_error_agree'] + stats['n_razor'] == s.n_targets and stats['n_exact'] > 0 and stats['n_razor'] <= 1


def test_hostsim_given_oracle_cut(hostsim):
	"""Integer part of the pipeline (A3..A5b) in isolation: feed the oracle's CUT."""
	s, S = make_cases('crowded', 11)
	from oracle import k2p2 as ok2p2
	cuts = np.full(s.n_targets, np.nan)
	for i in range(s.n_targets):
		try:
			cuts[i] = ok2p2.threshold(S[i], 0.8)
		except Exception: # noqa: B902
			cuts[i] = np.nan
	ok = np.isfinite(cuts)
	cuts[~ok] = 1e30
	got = run_hostsim(hostsim, s, S, cut_override=cuts)
	ref = oracle_batch(s, S, cut_override=cuts)
	compare(s, S, got, ref, check_cut=False)


def test_hostsim_two_sample_kde_tie(hostsim):
	"""A sum image with TWO positive pixels (fuzz scene 'bright' 338, target 4): the KDE has two maxima of equal height and the
	first argmax of the FFT density is decided by the transform's rounding noise -- the kernel's radix-2 FFT and numpy's land on
	different bumps, the thresholds differ (0.174 against 0.016), and every OUTPUT is the same: no cluster either way, minimum
	aperture, STATUS.WARNING.  `compare` counts it as a tie and still checks the outputs."""
	s, S = make_cases('bright', 338)
	stats = compare(s, S, run_hostsim(hostsim, s, S), oracle_batch(s, S))
	assert stats['n_tie'] == 1 and stats['n_razor'] == 0   # (compare itself asserts status, mask, flags, contamination of every target)


def test_hostsim_kde_argmax_on_large_stamps(hostsim):
	"""Stamps with more than 512 (and more than 1 024) positive pixels: the linear binning of the KDE -- run boundaries by binary search
	in the sorted sample -- must make enough halvings for the sample size.  Nine (enough for 16 x 16 pixels) were made for every stamp
	until round 6: the KDE's argmax came out a grid step off on some 45 x 50 stamps while CUT, after the Powell search, still agreed
	to 2e-7 -- so the argmax itself is asserted (k2p2_common.compare)."""
	from photometry_amd import simulate
	from oracle import sumimage as osum
	for (H, W, seed) in [(45, 50, 2), (40, 40, 1)]:
		s = simulate.make_scene(12, 40, H, W, seed=seed, max_neighbours=14, neighbour_tmag_range=(7.5, 13.5))
		simulate.fill_cubes(s)
		S = osum.sumimage_batch(s.images, s.quality)
		got = run_hostsim(hostsim, s, S)
		ref = oracle_batch(s, S)
		assert max(r['thr']['nflux_cut'] for r in ref if r.get('thr')) > (1024 if H * W > 2000 else 512)
		stats = compare(s, S, got, ref)
		assert stats['n_exact'] + stats['n_error_agree'] + stats['n_razor'] == s.n_targets and stats['n_exact'] >= 10


@pytest.mark.parametrize("H,W", [(9, 9), (10, 11), (11, 11), (12, 12), (13, 13), (13, 14), (8, 16)])
def test_hostsim_crowded_small_stamps(hostsim, H, W):
	"""Crowded stamps of 66 - 191 pixels, several clusters each: the sizes at which the scratch of the per-cluster bounding box once
	overlapped other per-lane scratch (the KDE grid of A2 shares its memory with A4's arrays) -- a window that comes out too small drops
	peaks, and the masks differ from the oracle's."""
	from photometry_amd import simulate
	from oracle import sumimage as osum
	s = simulate.make_scene(40, 30, H, W, seed=100 + H * W, max_neighbours=6, neighbour_tmag_range=(8.0, 13.0))
	simulate.fill_cubes(s)
	S = osum.sumimage_batch(s.images, s.quality)
	got = run_hostsim(hostsim, s, S)
	ref = oracle_batch(s, S)
	stats = compare(s, S, got, ref)
	assert stats['n_exact'] + stats['n_error_agree'] + stats['n_razor'] == s.n_targets and stats['n_exact'] >= 30 and stats['n_razor'] <= 1
