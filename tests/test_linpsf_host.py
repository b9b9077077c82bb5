# -*- coding: utf-8 -*-
"""
CPU-only checks of the designed LinPSF cases (``linpsf_common.CASES``): what the device tests rely on is asserted here on the
inputs and on the oracle -- the star selection on permuted catalogues, each row's design facts and the counters they imply, the
conditioning of the oracle's normal matrix (so that a comparison at 1e-8 means something), the distance of every contamination
from the warning threshold (so that a status mismatch is a defect and not a rounding flip), and that permuting a catalogue
changes nothing but the order.
"""
import numpy as np
import pytest

import linpsf_common as lc

#: the rows with series of thousands of cadences are checked by design facts only: their oracle runs take minutes on the CPU
LONG = ('cadences_4096', 'cadences_4097')
ORACLE_ROWS = [n for n in lc.CASES if n not in LONG]


def test_select_stars_on_permuted_catalogues():
	"""``psf.select_stars`` against ``oracle.linpsf.select_stars``: the target at every position of its slice, rejected stars ahead."""
	from photometry_amd import simulate, psf as hpsf
	from oracle import linpsf as olin
	seen = set()
	for seed in range(6):
		for place in ('front', 'middle', 'end', 'random'):
			s = simulate.make_scene(7, 4, 13, 13, seed=300 + seed, max_neighbours=5, neighbour_tmag_range=(8.0, 19.0))
			rng = np.random.default_rng([seed, 1])
			lc.add_rejected(s, rng)
			lc.permute_catalog(s, rng, place)
			sel, star_offsets, target_index = hpsf.select_stars(s.catalog, s.cat_offsets, s.target_starid)
			for i in range(s.n_targets):
				a, b = s.cat_offsets[i], s.cat_offsets[i + 1]
				indx, staridx = olin.select_stars(s.catalog_of(i), s.target_starid[i])
				np.testing.assert_array_equal(sel[a:b], indx)
				assert star_offsets[i + 1] - star_offsets[i] == indx.sum() and target_index[i] == int(staridx)
				cat_index = int(np.flatnonzero(s.catalog['starid'][a:b] == s.target_starid[i])[0])
				seen.add((int(indx.sum()), int(staridx), cat_index != int(staridx)))
	# the target first, in the middle, last; and a fitted index that differs from the catalogue index
	assert any(n >= 3 and 0 < t < n - 1 for (n, t, _) in seen) and any(n >= 2 and t == n - 1 for (n, t, _) in seen) and any(t == 0 for (_, t, _) in seen)
	assert any(d for (_, _, d) in seen)


def test_designed_catalogues_select_as_designed():
	"""Every row: the selection keeps exactly the designed stars, the target at its designed place, the rejected ones ahead of it."""
	from oracle import linpsf as olin
	for name in lc.CASES:
		case = lc.build_case(name)
		s = case['scene']
		for i, sp in enumerate(s.specs):
			assert case['star_offsets'][i + 1] - case['star_offsets'][i] == sp['S'], (name, i)
			assert case['target_index'][i] == sp['place'], (name, i)
			indx, staridx = olin.select_stars(s.catalog_of(i), s.target_starid[i])
			assert np.flatnonzero(indx).tolist() == sp['fitted'] and int(staridx) == sp['place']
			assert sp['fitted'][sp['place']] != sp['place']          # the catalogue index differs from the fitted index


@pytest.mark.parametrize("name", list(lc.CASES))
def test_row_reaches_its_class(name):
	"""The counters a row asserts on the device follow from the host restatement of the plan kernel at its designed positions."""
	case = lc.build_case(name)
	row = case['row']
	if row.get('kind', 'spoc') != 'spoc' or row.get('cutoff', 5) is None:
		# not the SPOC layout with the plugin's cut-off: every target on the any-grid kernels (tp_linpsf_grid_kernel decides)
		assert lc.case_counts(case, 1) == lc.expected_counts([None] * case['scene'].n_targets, any_grid=True)
		return
	for path in row['paths']:
		assert lc.case_counts(case, path) == lc.expected_counts(lc.case_classes(case, path)), (name, path)


def test_design_facts():
	_, model = lc.prf_and_model()
	# the (na, nb) shapes of the one-segment matrix-core row: (1,1), the 2 x 2 packing, (3,3) and a mixed shape for every star count
	case = lc.build_case('matrix_shapes')
	cl = lc.case_classes(case, 1)
	so = case['star_offsets']
	for i, want in enumerate(case['row']['facts']['shapes']):
		for s in range(so[i], so[i + 1]):
			assert lc.intervals_visited(model, case['pos_row'][s], case['pos_col'][s], 0, 2) == want, (i, s)
	small, large = case['row']['facts']['lds_over_small'], case['row']['facts']['lds_over_large']
	# three stars, 3 x 3 intervals: 18 (star, pixel tile) pairs x 13 steps x 512 B = 119 808 B, beyond "small", inside "large"
	assert cl[small]['stars'] == 3 and cl[small]['shapes'] == [[(3, 3)] * 3] and cl[small]['lds'] == [119808]
	assert lc.MFMA_LDS_SMALL < cl[small]['lds'][0] <= lc.MFMA_LDS_LARGE and cl[small]['cls'] == 'matrix'
	# four stars, 3 x 3 intervals: 173 056 B, beyond "large" -> the vector-ALU kernels
	assert cl[large]['stars'] == 4 and cl[large]['lds'] == [173056] and cl[large]['lds'][0] > lc.MFMA_LDS_LARGE and cl[large]['cls'] == 'poly'
	assert lc.mfma_steps(2, 2) == 9 and lc.mfma_steps(3, 3) == 13 and lc.mfma_steps(1, 1) == 7 and lc.mfma_steps(3, 2) == 11
	# segments: 1, 2, 8 -- and 9, which is one too many
	case = lc.build_case('segments_333')
	for i, want in enumerate(case['row']['facts']['n_segments']):
		pr, pc = case['pos_row'][so_slice(case, i)], case['pos_col'][so_slice(case, i)]
		assert len(lc.segments(model, pr, pc, limit=99)) == want, i
		assert (lc.segments(model, pr, pc) is None) == (want > lc.MFMA_SEGS)
		assert max(lc.origin_count(model, r, c) for r, c in zip(pr, pc)) <= lc.MAX_ORIGINS       # ... so the ninth leaves for fit2, not for the direct kernel
	# the union list: 255 pixels on the matrix cores, 257 off them -- and nothing else takes them off
	for name in ('union_under', 'union_over'):
		case = lc.build_case(name)
		for i, want in enumerate(case['row']['facts']['n_pix']):
			pr, pc = case['pos_row'][so_slice(case, i)], case['pos_col'][so_slice(case, i)]
			n_pix, tiles = lc.union_plan(pr, pc, 21, 21)
			assert n_pix == want and (tiles is None) == (want > lc.MFMA_PIXELS)
			assert len(lc.segments(model, pr, pc)) == 3
			# counted again, literally: pixels nearer than the cut-off to the rectangle some star's position sweeps
			n = 0
			for r in range(21):
				for c in range(21):
					d2 = [max(0.0, a.min() - r, r - a.max())**2 + max(0.0, b.min() - c, c - b.max())**2 for a, b in zip(pr, pc)]
					n += min(d2) < 25.0
			assert n == want
	# the direct kernel's rows: more than 36 table origins for every star
	case = lc.build_case('direct_1to8')
	for s in range(len(case['pos_row'])):
		assert lc.origin_count(model, case['pos_row'][s], case['pos_col'][s]) > lc.MAX_ORIGINS
	case = lc.build_case('valu_1to8')
	assert np.diff(case['star_offsets']).tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
	assert np.diff(lc.build_case('many')['star_offsets']).tolist() == [9, 33, 64]
	# the stretch of NaN positions covers whole tiles of cadences; the star that leaves does so at a tile boundary
	case = lc.build_case('edge_nan_stretch')
	sp = case['scene'].specs[1]
	nb = sp['fitted'][(sp['place'] + 1) % sp['S']]
	assert lc.intervals_visited(model, sp['pos'][:, nb, 0], sp['pos'][:, nb, 1], 1, 2) == (0, 0)
	assert lc.intervals_visited(model, sp['pos'][:, nb, 0], sp['pos'][:, nb, 1], 0, 1) == (2, 2)
	# ... and with the staircase under it every tile is a segment: the neighbour has na == 0 in the second of three segments only
	case = lc.build_case('edge_nan_segment')
	for i in (0, 1, 2):
		cl = lc.case_classes(case, 1)[i]
		assert cl['cls'] == 'matrix' and cl['segments'] == [(0, 1), (1, 2), (2, 3)]
		nb = (case['scene'].specs[i]['place'] + 1) % cl['stars']
		assert [sh[nb] for sh in cl['shapes']] == [(1, 1), (0, 0), (1, 1)] and all(sh[case['scene'].specs[i]['place']] == (1, 1) for sh in cl['shapes'])
	# a star with na == 0 has no blocks in its segment's coefficient image: in target 1 it is the LAST fitted star, whose blocks would
	# begin where the image ends -- the fit must not read there (whatever lies in LDS behind the image, times zero, may be NaN)
	last = [(case['scene'].specs[i]['place'] + 1) % case['scene'].specs[i]['S'] == case['scene'].specs[i]['S'] - 1 for i in (0, 1, 2)]
	assert last == [False, True, False]


def so_slice(case, i):
	return slice(int(case['star_offsets'][i]), int(case['star_offsets'][i + 1]))


def _normal_matrices(case, i, cadences):
	"""The oracle's ``A^T A`` of target ``i`` at the given cadences (every pixel of the stamp: NaN pixels only remove rows)."""
	from oracle import psf as opsf
	row, s = case['row'], case['scene']
	prf, _ = lc.prf_and_model(row.get('kind', 'spoc'))
	p = opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(s.stamps[i]))
	sp = s.specs[i]
	out = []
	for k in cadences:
		good = np.isfinite(lc.oracle_images(case, i)[:, :, k])
		A = np.stack([p.integrate_to_image(np.atleast_2d([sp['pos'][k, c, 0], sp['pos'][k, c, 1], 1.0]), cutoff_radius=row.get('cutoff', 5))[good]
			for c in sp['fitted']], axis=1)
		out.append(A.T @ A)
	return out


@pytest.mark.parametrize("name", ORACLE_ROWS + list(LONG))
def test_conditioning(name):
	"""Every eigenvalue of the oracle's normal matrix above 1e-9 of the largest at the first, a middle and the last cadence -- or, where
	a row is singular by design, singular EXACTLY: zero columns, and the rest of the matrix as well conditioned as elsewhere."""
	case = lc.build_case(name)
	s = case['scene']
	T = s.n_cad
	for i in range(s.n_targets):
		for k, G in zip((0, T // 2, T - 1), _normal_matrices(case, i, (0, T // 2, T - 1))):
			zero = np.flatnonzero(np.all(G == 0.0, axis=0))
			if len(zero) == len(G):
				continue         # a frame without a good pixel: the zero matrix (flux 0 by pinv)
			live = np.setdiff1d(np.arange(len(G)), zero)
			w = np.linalg.eigvalsh(G[np.ix_(live, live)])
			assert w.min() > 1e-9 * w.max(), (name, i, k, w.min() / w.max())
			if len(zero):
				# exactly zero columns only where the design says so: a star never / no longer on the stamp, a NaN position
				pos = s.specs[i]['pos'][k][s.specs[i]['fitted']][zero]
				assert np.all(~np.isfinite(pos).all(axis=1) | ~np.array([lc.on_stamp(q[:1], q[1:], s.height, s.width) for q in pos])), (name, i, k)


@pytest.mark.parametrize("name", ORACLE_ROWS)
def test_status_margins(name):
	"""Every target's oracle contamination is at least 1e-3 away from the 0.1 warning threshold, its fluxes finite."""
	case = lc.build_case(name)
	for i, ref in enumerate(lc.oracle_case(case)):
		assert np.all(np.isfinite(ref['flux'])) and np.all(np.isfinite(ref['fluxes_all'])), (name, i)
		assert abs(ref['contamination'] - 0.1) >= 1e-3, (name, i, ref['contamination'])
		np.testing.assert_array_equal(ref['fluxes_all'][:, ref['staridx']], ref['flux'])


@pytest.mark.parametrize("name", ['tail_15', 'edge_nan_both', 'valu_1to8'])
def test_oracle_is_invariant_under_permutation(name):
	"""The oracle on a permuted catalogue equals the oracle on the designed one to 1e-12: the permutation helper changes the order
	and nothing else."""
	import copy
	from oracle import psf as opsf, linpsf as olin
	case = lc.build_case(name)
	refs = lc.oracle_case(case)
	s = copy.copy(case['scene'])
	s.catalog = {k: v.copy() for k, v in s.catalog.items()}
	s.positions = [p.copy() for p in s.positions]
	lc.permute_catalog(s, np.random.default_rng(8), 'random')
	prf, _ = lc.prf_and_model()
	moved = 0
	for i in range(s.n_targets):
		cat = s.catalog_of(i)
		p = opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(s.stamps[i]))
		got = olin.do_photometry(s.images[i], p, cat, s.target_starid[i], s.positions[i], tuple(s.stamps[i]), s.target_pos_row[i], s.target_pos_column[i], s.aperture[i])
		ref = refs[i]
		scale = np.nanmax(np.abs(ref['flux']))
		np.testing.assert_allclose(got['flux'], ref['flux'], rtol=1e-12, atol=1e-12 * scale)
		np.testing.assert_allclose(got['contamination'], ref['contamination'], rtol=1e-12, atol=1e-15)
		# the fitted stars in their new order
		old = case['scene'].catalog_of(i)['starid'][ref['indx']]
		new = cat['starid'][got['indx']]
		order = [int(np.flatnonzero(old == x)[0]) for x in new]
		np.testing.assert_allclose(got['fluxes_mean'], ref['fluxes_mean'][order], rtol=1e-12, atol=1e-12 * scale)
		moved += int(got['staridx'] != ref['staridx'])
	assert moved > 0
