# -*- coding: utf-8 -*-
"""
Every LinPSF fit class against the oracle, the target anywhere in its list of fitted stars.

The rows of ``linpsf_common.CASES`` are targets built by design (star count, place of the target, knot intervals visited, series
length, pixels within reach): each row names the class of ``linpsf_fit_impl``'s dispatch it reaches and the counters of
``tp_linpsf_last_counts`` that prove it (asserted exactly; ``test_linpsf_host.py`` derives the same counters on the CPU from a
restatement of the plan kernel).  Every target of every row is compared with ``oracle.linpsf.do_photometry`` in full: flux,
``fluxes_mean``, contamination, status, ``flux_err`` NaN, and ``fluxes_all`` of every fitted star at every cadence, at the
tolerances of ``test_gpu_linpsf.py``.
"""
import numpy as np
import pytest

import linpsf_common as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _rows(*names):
	return [(n, p) for n in names for p in lc.CASES[n]['paths']]


def _placed(case):
	"""Every row has a target whose index in its fitted list is not 0; with three and more stars one in the middle and one last."""
	ti, ns = case['target_index'], np.diff(case['star_offsets'])
	assert np.any(ti > 0), case['name']
	if np.any(ns >= 3):
		assert np.any((ns >= 3) & (ti == ns - 1)) and np.any((ns >= 3) & (ti > 0) & (ti < ns - 1)), case['name']


# 1. matrix-core classes of 1..4 stars in one segment, (na, nb) = (1,1), (2,2) -- the 9-step packing --, (3,3), (1,3) / (3,2);
#    the three-star (3,3) image beyond kMfmaLdsSmall, the four-star one beyond kMfmaLdsLarge (-> vector ALU)
# 2. 1 / 2 / 8 segments, a ninth -> vector ALU; series of 1, 15, 16, 17, 333 cadences; 4096 on the matrix cores, 4097 off them
# 3. union list of 255 pixels on the matrix cores, 257 off them
# 4. fit2<1,0> <2,2> <3,3> <4,4> <8,5> (5, 6, 7, 8 stars); fit_direct<2,0> <4,3> <8,5> (more than 36 origins)
# 5. the many-star kernel: 9, 33, 64 stars, the target first, in the middle, last
# 6. the any-grid kernels: 2, 5, 12 stars
@pytest.mark.parametrize("name,path", _rows('matrix_shapes', 'segments_333', 'tail_1', 'tail_15', 'tail_16', 'tail_17', 'cadences_4096', 'cadences_4097',
	'union_under', 'union_over', 'valu_1to8', 'direct_1to8', 'many', 'anygrid_rect', 'anygrid_nocut'))
def test_class_matches_oracle(ctx, name, path):
	case = lc.build_case(name)
	if name not in ('cadences_4096', 'cadences_4097'):
		_placed(case)
	else:
		assert np.any(case['target_index'] > 0)
	lc.run_and_compare(ctx, case, path)


def test_more_than_64_stars_is_refused(ctx):
	"""65 fitted stars: the documented error, by the argument check (max_stars) and by the per-target check (star offsets)."""
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	from photometry_amd._lib import TessphotError
	_, model = lc.prf_and_model()
	T = 4
	img = DeviceCube(ctx, 1, T, 21, 21)
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(np.array([[10, 31, 60, 81]]))))
	pos = ctx.array(np.full((65, T), 10.0))
	for max_stars in (65, 64):      # 64: the argument passes, the target's own count does not
		with pytest.raises(TessphotError) as e:
			engine.linpsf_fit(ctx, img, coef, ctx.array(model.tx), ctx.array(model.ty), ctx.array(np.array([0, 65], dtype='int64')),
				ctx.array(np.array([64], dtype='int32')), pos, pos, max_stars)
		assert '64' in str(e.value) and 'stars' in str(e.value)


# 7. every class in one call, interleaved
@pytest.mark.parametrize("path", [0, 1])
def test_mixed_batch(ctx, path):
	"""23 targets of every class in ONE call: the class lists, segment lists and store offsets are per-batch indexing.  Each target is
	compared with the oracle AND with a call of its own: bit for bit -- no kernel sums across targets, and a target's cadence
	order, pixel order and coefficient arithmetic do not depend on what else is in the batch."""
	case = lc.build_case('mixed')
	s = case['scene']
	assert s.n_targets == 23
	_placed(case)
	res, counts = lc.run_and_compare(ctx, case, path)
	classes = lc.case_classes(case, path)
	if path == 1:
		assert {c['cls'] for c in classes} == {'matrix', 'poly', 'direct', 'many'}
		assert counts['matrix_core_segments'] > counts['matrix_core_targets'] and min(counts['matrix_core_targets_by_stars']) > 0
	so = case['star_offsets']
	for i in range(s.n_targets):
		own, own_counts, _ = lc.run_case(ctx, case, path, targets=[i])
		assert own_counts == lc.expected_counts([classes[i]]), (i, own_counts)
		for k in ('flux', 'flux_err', 'contamination', 'status'):
			np.testing.assert_array_equal(own[k][0], res[k][i], err_msg=f'target {i} {k}')
		np.testing.assert_array_equal(own['fluxes_all'][:so[i + 1] - so[i]], res['fluxes_all'][so[i]:so[i + 1]], err_msg=f'target {i} fluxes_all')
		np.testing.assert_array_equal(own['fluxes_mean'][:so[i + 1] - so[i]], res['fluxes_mean'][so[i]:so[i + 1]], err_msg=f'target {i} fluxes_mean')


# 8. data edges, each on a matrix-core class (path 1) = a fit2 class (path 0) of 2 and 3 stars, on fit2<8,5> (6 stars) and on the
#    many-star kernel (10 stars)
@pytest.mark.parametrize("name,path", _rows('edge_leaves', 'edge_never', 'edge_nan_row', 'edge_nan_col', 'edge_nan_both', 'edge_nan_stretch', 'edge_nan_segment',
	'edge_last_frame_nan', 'edge_last_frame_centre_nan', 'edge_nan_pixel_column', 'edge_subtract'))
def test_data_edge_matches_oracle(ctx, name, path):
	case = lc.build_case(name)
	_placed(case)
	res, _ = lc.run_and_compare(ctx, case, path)
	if name == 'edge_never':
		# the neighbour that no pixel ever sees: an exactly zero column, flux exactly 0 at every cadence
		so = case['star_offsets']
		for i, sp in enumerate(case['scene'].specs):
			nb = (sp['place'] + 1) % sp['S']
			assert np.all(res['fluxes_all'][so[i] + nb, :case['scene'].n_cad] == 0.0), i
	if name == 'edge_last_frame_nan':
		assert np.all(res['flux'][:, case['scene'].n_cad - 1] == 0.0)


@pytest.mark.parametrize("path", [0, 1])
def test_pitches_beyond_the_series(ctx, path):
	"""``pos_pitch``, ``out_pitch`` and the cube's ``t_pitch`` larger than ``n_cad`` (and different from each other): same results as
	packed, the padding of the inputs never read into them and the padding of the outputs untouched."""
	case = lc.build_case('edge_pitches')
	s = case['scene']
	T = s.n_cad
	refs = lc.oracle_case(case)
	res, counts, offs = lc.run_case(ctx, case, path, pitches=(T + 5, T + 11, T + 3))
	assert counts == lc.case_counts(case, path)
	for i in range(s.n_targets):
		lc.compare_target(res, i, offs, refs[i], T, label=f'pitches path {path}')
	packed, _, _ = lc.run_case(ctx, case, path)
	for k in ('flux', 'flux_err', 'fluxes_all'):
		np.testing.assert_array_equal(res[k][:, :T], packed[k][:, :T])
		assert np.all(res[k][:, T:] == -12345.0), k          # the sentinel behind the series
	np.testing.assert_array_equal(res['contamination'], packed['contamination'])
	np.testing.assert_array_equal(res['cube_after'], res['cube_before'])


# 9. through the product layers
def test_plugin_with_a_permuted_catalogue(ctx, tmp_path):
	"""``LinPSFPhotometry`` over catalogues in which the target is at the front, in the middle and at the end of its slice, stars the
	selection rejects ahead of it: against the oracle on the same catalogue."""
	from photometry_amd import simulate, psf as hpsf
	from photometry_amd.source import source_from_scene
	from photometry_amd.plugins import LinPSFPhotometry
	from oracle import psf as opsf, linpsf as olin
	prf, model = lc.prf_and_model()
	seen = set()
	for place in ('front', 'middle', 'end'):
		s = simulate.make_scene(3, 14, 11, 11, seed=61, max_neighbours=3, neighbour_tmag_range=(9.0, 15.0))
		rng = np.random.default_rng(4)
		lc.add_rejected(s, rng)
		lc.permute_catalog(s, rng, place)
		simulate.fill_cubes(s, nan_fraction=0.005)
		for i in range(s.n_targets):
			src = source_from_scene(s, i)
			src.prf = model
			with LinPSFPhotometry(int(s.target_starid[i]), src, str(tmp_path), ctx=ctx) as pho:
				status = pho.do_photometry()
				cat = pho.catalog
				T = s.n_cad
				positions = np.empty((T, len(cat), 2))
				for k in range(T):
					ck = pho.catalog_attime(pho.lightcurve['time'][k] - pho.lightcurve['timecorr'][k])
					positions[k, :, 0] = ck['row_stamp']
					positions[k, :, 1] = ck['column_stamp']
				p = opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], pho.stamp)
				ref = olin.do_photometry(s.images[i], p, {k: np.asarray(cat[k]) for k in ('starid', 'tmag', 'row_stamp', 'column_stamp')},
					s.target_starid[i], positions, pho.stamp, pho.target_pos_row, pho.target_pos_column, np.ones((11, 11), dtype='int32'))
				seen.add((ref['nstars'], ref['staridx']))
				np.testing.assert_allclose(pho.lightcurve['flux'], ref['flux'], rtol=1e-8, atol=1e-9 * np.nanmax(np.abs(ref['flux'])))
				assert status.value == ref['status']
				np.testing.assert_allclose(pho.additional_headers['PSF_CONT'][0], ref['contamination'], rtol=1e-7, atol=1e-11)
	assert any(idx > 0 for (_, idx) in seen) and any(n >= 3 and 0 < idx < n - 1 for (n, idx) in seen) and any(n >= 2 and idx == n - 1 for (n, idx) in seen), seen


def test_linpsf_frames_with_a_permuted_catalogue(tmp_path):
	"""``pipeline.linpsf_frames`` over a region whose catalogue lists the targets AFTER their neighbours: the same light curves,
	contamination and status as the plugin, target by target (as test_gpu_psf_frames.py / test_gpu_wcs.py compare them)."""
	from test_gpu_psf_frames import _region
	from photometry_amd import pipeline, psf as hpsf, simulate, STATUS
	from photometry_amd.device import Context
	from photometry_amd.plugins import LinPSFPhotometry
	from photometry_amd.source import MemoryStampSource
	T = 12
	frames, row0, col0, time, quality, cat, targets, jitter = _region(T=T)
	perm = np.arange(len(cat['starid']))[::-1].copy()       # blends: (0, 1) -> the fainter first; the three-star group reversed
	perm[[2, 3]] = perm[[3, 2]]                             # ... and then its middle star moved: every place occurs
	cat = {k: v[perm] for k, v in cat.items()}
	prf = simulate.synthetic_prf(seed=3)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	ctx = Context(0)
	try:
		stack = pipeline.FrameStack(ctx, {k: np.moveaxis(v, 2, 0) for k, v in frames.items()}, row0, col0)
		src = MemoryStampSource(frames, row0, col0, time, np.zeros(T), np.arange(T), quality, cat, targets=targets, jitter=jitter, prf=model)
		batch = pipeline.linpsf_frames(ctx, stack, targets, cat, time, quality, model, jitter=jitter)
		places = set()
		for i in range(len(targets['starid'])):
			b = batch[i]
			with LinPSFPhotometry(int(targets['starid'][i]), src, str(tmp_path), ctx=ctx) as pho:
				status = pho.do_photometry()
				c = pho.catalog
				sel, so, ti = hpsf.select_stars({k: np.asarray(c[k]) for k in ('starid', 'tmag', 'row_stamp', 'column_stamp')}, np.array([0, len(c)]), np.array([pho.starid]))
				places.add((int(so[1]), int(ti[0])))
				assert tuple(pho.stamp) == b['stamp'] and status.value == b['status']
				np.testing.assert_array_equal(pho.lightcurve['flux'], b['flux'])
				if status != STATUS.ERROR:
					assert pho.additional_headers['PSF_CONT'][0] == b['contamination']
		assert any(t > 0 for (_, t) in places), places
	finally:
		ctx.close()
