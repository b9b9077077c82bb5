# -*- coding: utf-8 -*-
"""
No GPU: what tests/test_gpu_extract_variants.py relies on, asserted on the oracle and on the kernel's own layout function.

* The Python restatement of where ``k.lab`` lies (extract_variants_common.offset_of_lab), from which every cadence count of the seam
  tests is derived, equals ``k2p2::shared_carve`` (host build, tests/hostsim/k2p2_hostsim.cpp) for every stamp from 1 x 1 to 54 x 54.
* Every hand-made target has a mask of the intended size; the raw scenes give their targets masks.
* For every mode and every class of mask sizes of the seam tests, cadence counts on BOTH sides of the seam between the LDS-staged and
  the HBM-series form of ``extract_small_stream`` are among the chosen ones -- no trace shows which form ran (both are inlined in
  one kernel), so this is the evidence that both did.  Every target of the long scenes takes the HBM-series form.
"""
import numpy as np
import pytest
import extract_variants_common as evc


def test_offset_of_lab_is_the_kernels():
	for H in range(1, 55):
		for W in range(1, 55):
			assert evc.offset_of_lab(H, W) == evc.hostsim_offset_of_lab(H, W), (H, W)


def test_room_is_positive_for_every_list_the_kernel_streams():
	"""The table of a mask of up to 128 pixels ends before the list (fused.hip: 'at least 3 072 bytes in ... the table takes 2 560')."""
	for H in range(1, 55):
		for W in range(1, 55):
			assert evc.room(H, W, min(H * W, 128)) >= 0, (H, W)


@pytest.mark.parametrize("H,W", evc.SEAM_STAMPS)
def test_seam_targets_have_the_intended_masks(H, W):
	b = evc.seam_batch(H, W)
	sizes = evc.mask_sizes(b)
	for i, n in enumerate(sizes):
		assert 1 <= n <= 128, (i, n)                      # (all of them take the streamed extraction)
		assert b.expected[i] is None or n == b.expected[i], (i, n, b.expected[i])
	assert set(sizes) >= ({1, 7, 8, 9, 16, 17, 128} if (H, W) == (15, 15) else {1, 7, 8, 9})
	# the classes: the pixel table is padded to whole groups of 8, so masks of 1..8, 9..16, ... share a room
	assert len(evc.seam_rooms(b)) == len({evc.round_up(n, 8) for n in sizes})


@pytest.mark.parametrize("H,W", evc.SEAM_STAMPS)
@pytest.mark.parametrize("mode", evc.SEAM_MODES)
def test_both_sides_of_the_seam_are_chosen(H, W, mode):
	b = evc.seam_batch(H, W)
	counts = evc.seam_counts(b, mode)
	ns = evc.n_series(mode)
	for aligned in (True, False):
		vec = evc.vec_of(aligned)
		for M in sorted({evc.round_up(n, 8) for n in evc.mask_sizes(b)}):
			sides = {evc.staged(H, W, M, T, vec, ns) for T in counts}
			if ns == 0:
				assert sides == {False}                       # no series: nothing to stage
			else:
				assert sides == {True, False}, (H, W, mode, aligned, M, counts)
	if ns:
		# ... and the counts sit AT the seam: the largest staged and the smallest unstaged count of a class are neighbours
		for aligned in (True, False):
			for M in sorted({evc.round_up(n, 8) for n in evc.mask_sizes(b)}):
				st = [T for T in counts if evc.staged(H, W, M, T, evc.vec_of(aligned), ns)]
				un = [T for T in counts if T > max(st) and not evc.staged(H, W, M, T, evc.vec_of(aligned), ns)]
				assert min(un) == max(st) + 1, (M, aligned, st, un)
	for T in counts:
		cpitch, spitch = evc.pitches(T, False)
		assert cpitch % 2 == 1 and spitch % 4 != 0 and cpitch >= T and spitch >= T
		assert cpitch == T or T % 2 == 0                      # (unpadded where the count is odd)


def test_big_masks_have_the_intended_sizes():
	b = evc.big_batch()
	sizes = evc.mask_sizes(b)
	assert sizes[:-1] == [s[3] for s in evc.BIG_STARS] and sizes[-1] == 9, sizes
	assert any(129 <= n <= 136 for n in sizes) and any(n > 256 for n in sizes)
	assert any(n > 128 and n % 8 != 0 for n in sizes) and any(n > 128 and n % 8 == 0 for n in sizes)
	for T in evc.BIG_T:
		for mode in evc.BIG_MODES:
			ref = evc.reference(b, evc.big_cubes(b, T, mode))
			flux = np.stack([r['flux'] for r in ref])
			assert np.isnan(flux).any() and np.isinf(flux).any() and (flux < 0).any() and np.isfinite(flux).any()
			assert np.isnan(np.stack([r['flux_background'] for r in ref])).any()


@pytest.mark.parametrize("name", sorted(evc.SCENES))
def test_instantiation_scenes_give_masks(name):
	shape = evc.SCENES[name]
	orc = evc.oracle_chain(shape)
	sizes = [int(o['ref']['mask'].sum()) for o in orc if o['ref']['status'] != 2 and o['ref']['mask'] is not None]
	print(f"{name}: {len(sizes)} of {shape[0]} targets with a mask, {min(sizes)} to {max(sizes)} pixels")
	assert 4 * len(sizes) >= 3 * shape[0]
	assert max(sizes) <= 128                                 # (the streamed extraction takes them)
	same, own = evc.scene_series(shape)
	assert np.isfinite(same).all() and not np.array_equal(same, own)


@pytest.mark.parametrize("name", sorted(evc.LONG_SCENES))
def test_long_scenes_take_the_hbm_series_form(name):
	n, T, H, W, _seed = shape = evc.LONG_SCENES[name]
	orc = evc.oracle_chain(shape)
	for i, o in enumerate(orc):
		assert o['ref']['status'] == 1 and o['ref']['mask'] is not None, (i, o['ref']['status'])
		M = int(o['ref']['mask'].sum())
		assert 1 <= M <= 128
		for vec in (1, 2):
			assert not evc.staged(H, W, M, T, vec, 1), (i, M)
