# -*- coding: utf-8 -*-
"""
GPU parity of the non-linear PSF photometry (``tp_psf_fit``; psf_photometry.py:52-108, 111-196) against the oracle, and
against the golden vectors produced by the reference's own ``PSFPhotometry.do_photometry`` (real scipy Nelder-Mead).

A Nelder-Mead run is a chain of comparisons of chi^2 values: last-bit differences in the summation order can change single
steps, after which two runs walk different simplices to the same minimum.  The minimum itself is pinned far tighter than the
stopping tolerances suggest (fatol = 1e-4 on chi^2 forces a simplex of ~1e-8): the oracle run with its chi^2 summed in another
order reproduces its own fluxes to 7e-9 although the iteration counts change (measured), and the device
agrees with the oracle to 1e-7 and with the reference's golden to 7e-9.  Fluxes are compared at 1e-6 relative (north_star:
1e-5), positions at 2e-6 pixels; the number of iterations is compared loosely, and a cadence may be finite on one side and
NaN on the other only when at least one of the two walks ran into its iteration limit (psf_photometry.py:190-194: "success" is
"finished before maxiter", a property of the walk, not of the minimum: the other walk may have converged hundreds of iterations
earlier -- 335 against 500, 815 against 1 500 in the committed distribution).  ``test_psf_parity_by_distribution`` asserts the
agreement as a distribution over 120 targets x 20 cadences against a committed oracle fixture.  The device's own Nelder-Mead is additionally pinned step for step: with the likelihood of a one-star target
the iteration counts match scipy's exactly until the first such flip in a target's warm-start chain.
"""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLUX_RTOL = 1e-6   # north_star: light-curve flux within 1e-5 relative; measured: <= 1e-7 (oracle), <= 7e-9 (reference golden)
POS_ATOL = 2e-6    # pixels; measured <= 2e-7


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _run_device(ctx, images, backgrounds, model, stamps, catalogs, pos_row, pos_col, tmag, apertures, **kw):
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	from photometry_amd.plugins import psf_star_selection, mag2flux
	from oracle.aperture import minimum_aperture
	Nt, H, W, T = images.shape
	offs, params, mini = [0], [], []
	for i in range(Nt):
		c = catalogs[i]
		sel = psf_star_selection(c['row_stamp'], c['column_stamp'], c['tmag'], pos_row[i] - stamps[i][0], pos_col[i] - stamps[i][2], tmag[i])
		params.append(np.column_stack((c['row_stamp'][sel].astype('float64'), c['column_stamp'][sel].astype('float64'), mag2flux(c['tmag'][sel].astype('float64')))))
		offs.append(offs[-1] + len(sel))
		mini.append(minimum_aperture(tuple(stamps[i]), pos_row[i], pos_col[i], apertures[i]))
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(stamps)))
	res = engine.psf_fit(ctx, DeviceCube.from_host(ctx, images), DeviceCube.from_host(ctx, backgrounds), coef, ctx.array(model.tx), ctx.array(model.ty),
		ctx.array(np.asarray(offs, dtype='int64')), ctx.array(np.concatenate(params)), ctx.array(np.stack(mini).astype('uint8')), **kw)
	return {k: v.to_host() for k, v in res.items()}


def test_psf_photometry_golden(ctx, golden_dir):
	from photometry_amd import psf as hpsf
	from scipy.interpolate import RectBivariateSpline
	g = np.load(os.path.join(golden_dir, 'golden_psfphot.npz'))
	x = g['prf_x']
	model = hpsf.PRFModel.from_spline(RectBivariateSpline(x, x, g['prf_img']))
	Nt = g['images'].shape[0]
	cats = []
	for i in range(Nt):
		a, b = g['cat_offsets'][i], g['cat_offsets'][i + 1]
		cats.append({k[4:]: g[k][a:b] for k in g.files if k.startswith('cat_') and k != 'cat_offsets'})
	res = _run_device(ctx, g['images'], g['backgrounds'], model, g['stamps'], cats, g['target_pos_row'], g['target_pos_column'],
		g['target_tmag'], g['aperture'])
	for n in range(int(g['n_psfphot'])):
		i = int(g[f'pp{n}_target'])
		ref = g[f'pp{n}_flux']
		ok = np.isfinite(ref)
		print('golden target', i, 'max rel flux diff', np.max(np.abs(res['flux'][i][ok] / ref[ok] - 1)), 'max pos diff',
			np.nanmax(np.abs(np.column_stack((res['centroid_row'][i], res['centroid_col'][i])) - g[f'pp{n}_pos_centroid'])))
		np.testing.assert_allclose(res['flux'][i], ref, rtol=FLUX_RTOL)
		np.testing.assert_allclose(np.column_stack((res['centroid_row'][i], res['centroid_col'][i])), g[f'pp{n}_pos_centroid'], atol=POS_ATOL)
		assert np.all(np.isnan(res['flux_err'][i])) and int(res['status'][i]) == int(g[f'pp{n}_status'])
		np.testing.assert_array_equal(res['flux_err'][i], g[f'pp{n}_flux_err'])   # NaN upstream (psf_photometry.py:175)


def test_psf_photometry_matches_oracle(ctx):
	from photometry_amd import simulate, psf as hpsf
	from oracle import psf as opsf, psf_photometry as opp
	Nt, T, H, W = 5, 6, 11, 11
	s = simulate.make_scene(Nt, T, H, W, seed=91, max_neighbours=3, neighbour_tmag_range=(9.0, 15.0))
	simulate.fill_cubes(s, nan_fraction=0.004)
	s.images[1, :, :, 2] = np.nan      # a frame without data: chi^2 = 0 everywhere, the simplex collapses by shrinking
	prf = opsf.synthetic_prf(seed=5)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	cats = [s.catalog_of(i) for i in range(Nt)]
	res = _run_device(ctx, s.images, s.backgrounds, model, s.stamps, cats, s.target_pos_row, s.target_pos_column, s.target_tmag, s.aperture)
	n_same_nit = n_cad = n_flag_diff = 0
	for i in range(Nt):
		p = opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(s.stamps[i]))
		ref = opp.do_photometry(s.images[i], s.backgrounds[i], p, cats[i], tuple(s.stamps[i]), s.target_pos_row[i], s.target_pos_column[i],
			s.target_tmag[i], s.aperture[i])
		# a run that needs about as many iterations as its limit (500) can finish on one side and not on the other: such a
		# cadence is NaN on that side only (psf_photometry.py:190-194); compared are the cadences both sides finished
		ok = ref['success'] & ~np.isnan(res['flux'][i])
		differ = np.flatnonzero(ref['success'] != ~np.isnan(res['flux'][i]))
		n_flag_diff += len(differ)
		for k in differ:
			# only a fit that runs into its iteration limit on one side may be finite on the other
			limit = 1500 if k == 0 else 500
			assert max(int(res['nit'][i][k]), int(ref['nit'][k])) >= limit, (i, k, res['nit'][i][k], ref['nit'][k])
		print(i, 'nit device', res['nit'][i], 'oracle', ref['nit'], 'success', ref['success'])
		if ok.any():
			print('   max rel flux diff', np.max(np.abs(res['flux'][i][ok] / ref['flux'][ok] - 1)), 'max pos diff',
				max(np.max(np.abs(res['centroid_row'][i][ok] - ref['pos_centroid'][ok, 0])), np.max(np.abs(res['centroid_col'][i][ok] - ref['pos_centroid'][ok, 1]))))
		np.testing.assert_allclose(res['flux'][i][ok], ref['flux'][ok], rtol=FLUX_RTOL)
		np.testing.assert_allclose(res['centroid_row'][i][ok], ref['pos_centroid'][ok, 0], atol=POS_ATOL)
		np.testing.assert_allclose(res['centroid_col'][i][ok], ref['pos_centroid'][ok, 1], atol=POS_ATOL)
		n_same_nit += int(np.sum(res['nit'][i] == ref['nit']))
		n_cad += T
	assert n_flag_diff <= 1
	# the device walks scipy's simplex: until the first last-bit flip in a target's warm-start chain the iteration counts are scipy's
	print(f"identical iteration counts on {n_same_nit} of {n_cad} cadences")
	assert n_same_nit >= n_cad // 4


@pytest.mark.parametrize("kind,cutoff", [('warped', 5), ('spoc', 6.5), ('nsub7', None), ('rect', 5)])
def test_psf_photometry_any_grid_any_cutoff(ctx, kind, cutoff):
	"""PRF grids other than the SPOC layout, cut-off radii beyond its evenly spaced knots or none (psf.py:119, :142): the general
	instantiation of the fit kernel integrates the spline over every pixel itself.  Same comparison as above."""
	from photometry_amd import simulate, psf as hpsf
	from oracle import psf as opsf, psf_photometry as opp
	from prf_common import general_prf
	Nt, T, H, W = 4, 4, 11, 11
	s = simulate.make_scene(Nt, T, H, W, seed=93, max_neighbours=2, neighbour_tmag_range=(9.0, 15.0))
	simulate.fill_cubes(s, nan_fraction=0.004)
	prf = general_prf(kind)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	cats = [s.catalog_of(i) for i in range(Nt)]
	res = _run_device(ctx, s.images, s.backgrounds, model, s.stamps, cats, s.target_pos_row, s.target_pos_column, s.target_tmag, s.aperture,
		cutoff_radius=cutoff)
	n_flag_diff = n_ok = 0
	for i in range(Nt):
		p = opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(s.stamps[i]))
		ref = opp.do_photometry(s.images[i], s.backgrounds[i], p, cats[i], tuple(s.stamps[i]), s.target_pos_row[i], s.target_pos_column[i],
			s.target_tmag[i], s.aperture[i], cutoff_radius=cutoff)
		ok = ref['success'] & ~np.isnan(res['flux'][i])
		differ = np.flatnonzero(ref['success'] != ~np.isnan(res['flux'][i]))
		n_flag_diff += len(differ)
		for k in differ:
			limit = 1500 if k == 0 else 500
			assert max(int(res['nit'][i][k]), int(ref['nit'][k])) >= limit, (i, k, res['nit'][i][k], ref['nit'][k])
		print(kind, cutoff, i, 'nit device', res['nit'][i], 'oracle', ref['nit'])
		np.testing.assert_allclose(res['flux'][i][ok], ref['flux'][ok], rtol=FLUX_RTOL)
		np.testing.assert_allclose(res['centroid_row'][i][ok], ref['pos_centroid'][ok, 0], atol=POS_ATOL)
		np.testing.assert_allclose(res['centroid_col'][i][ok], ref['pos_centroid'][ok, 1], atol=POS_ATOL)
		n_ok += int(ok.sum())
	assert n_flag_diff <= 1 and n_ok >= Nt * T // 2


def test_psf_parity_by_distribution(ctx, golden_dir):
	"""
	PSFPhotometry parity stated and asserted as a distribution: 120 targets x 20 cadences (one to three fitted stars, NaN pixels)
	against the committed fit of the oracle -- scipy's Nelder-Mead restated step for step on the FITPACK pixel integral, generated by
	tests/golden/make_psf_distribution.py (21 minutes on 7 processes).  A Nelder-Mead run is a chain of comparisons of chi^2 values:
	a last-bit difference in a sum sends the two sides along different simplices to the same minimum, so single cadences cannot
	be pinned tighter than the distribution: median |dflux| / flux <= 1e-8, 99 % <= 1e-6 (north_star: 1e-5), maximum <= 1e-3;
	finite / NaN pattern different on <= 3 % of the cadences, and ONLY where one of the two walks hit its iteration limit
	(psf_photometry.py:190-194: `success` is a property of the walk).
	"""
	import sys
	sys.path.insert(0, golden_dir)
	import make_psf_distribution as mk
	from photometry_amd import psf as hpsf
	g = np.load(os.path.join(golden_dir, 'golden_psf_distribution.npz'))
	Nt, T, H, W = (int(v) for v in g['shape'])
	assert (mk.NT, mk.T, mk.H, mk.W) == (Nt, T, H, W) and [mk.SCENE_SEED, mk.PRF_SEED] == [int(v) for v in g['seeds']]
	s, prf = mk.build_scene()
	assert float(np.nansum(s.images.astype('float64'))) == float(g['images_checksum'][0])      # the scene the oracle fitted
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	cats = [s.catalog_of(i) for i in range(Nt)]
	res = _run_device(ctx, s.images, s.backgrounds, model, s.stamps, cats, s.target_pos_row, s.target_pos_column, s.target_tmag, s.aperture)
	flux_d, flux_o = np.asarray(res['flux'])[:, :T], g['flux']
	nit_d, nit_o = np.asarray(res['nit'])[:, :T], g['nit']
	cen_d = np.stack((np.asarray(res['centroid_row'])[:, :T], np.asarray(res['centroid_col'])[:, :T]), axis=-1)
	fin_d, fin_o = np.isfinite(flux_d), np.isfinite(flux_o)
	limit = np.full((Nt, T), 500)
	limit[:, 0] = 1500
	differ = fin_d != fin_o
	both = fin_d & fin_o
	rel = np.abs(flux_d[both] / flux_o[both] - 1)
	dpos = np.abs(cen_d - g['pos_centroid'])[both].max(axis=1)
	n_cad = Nt * T
	pct = {q: float(np.percentile(rel, q)) for q in (50, 90, 99, 99.9, 100)}
	print(f'PSF parity: {int(both.sum())} cadences finite on both sides, {int(differ.sum())} on one side only ({100.0 * differ.sum() / n_cad:.2f} %)')
	print('   |dflux|/flux percentiles:', {k: f'{v:.2e}' for k, v in pct.items()}, ' |dpos| px: median %.2e, max %.2e' % (np.median(dpos), dpos.max()))
	print('   identical iteration counts: %.1f %%' % (100.0 * np.mean(nit_d[both] == nit_o[both])))
	assert both.sum() >= 0.4 * Nt * T      # (the rest: fits that run into maxiter on both sides -- NaN by the reference's rule)
	assert pct[50] <= 1e-8 and pct[99] <= 1e-6 and pct[100] <= 1e-3
	assert np.median(dpos) <= 1e-7 and np.percentile(dpos, 99) <= 2e-6
	assert differ.sum() <= 0.03 * n_cad
	hit = (nit_d >= limit) | (nit_o >= limit)
	bad = np.argwhere(differ & ~hit)
	assert len(bad) == 0, [(int(i), int(k), int(nit_d[i, k]), int(nit_o[i, k])) for i, k in bad]
	# the side that is NaN is the side that hit its limit
	assert np.all(nit_d[differ & ~fin_d] >= limit[differ & ~fin_d]) and np.all(nit_o[differ & ~fin_o] >= limit[differ & ~fin_o])


def test_psf_fit_batch_equals_target_by_target(ctx):
	"""The kernel launches the targets of a batch by their number of fitted stars (one to five, a coefficient pool sized for each
	class, three streams): every target gets exactly what it gets when fitted alone -- fluxes, centroids and iteration counts
	bit for bit -- and the classes with four and five stars are exercised."""
	from photometry_amd import simulate, engine, psf as hpsf
	from photometry_amd.device import DeviceCube
	from photometry_amd.plugins import psf_star_selection, mag2flux
	from oracle import psf as opsf
	Nt, T, H, W = 24, 3, 13, 13
	s = simulate.make_scene(Nt, T, H, W, seed=123, max_neighbours=6, neighbour_tmag_range=(9.0, 13.5))
	simulate.fill_cubes(s, nan_fraction=0.002)
	prf = opsf.synthetic_prf(seed=5)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	offs, params, mini = [0], [], []
	for i in range(Nt):
		c = s.catalog_of(i)
		sel = psf_star_selection(c['row_stamp'], c['column_stamp'], c['tmag'], s.target_pos_row[i] - s.stamps[i][0], s.target_pos_column[i] - s.stamps[i][2], s.target_tmag[i])
		params.append(np.column_stack((c['row_stamp'][sel].astype('float64'), c['column_stamp'][sel].astype('float64'), mag2flux(c['tmag'][sel].astype('float64')))))
		offs.append(offs[-1] + len(sel))
		m = np.zeros((H, W), dtype='uint8')
		r, cc = int(round(s.target_pos_row[i] - s.stamps[i][0])), int(round(s.target_pos_column[i] - s.stamps[i][2]))
		m[max(r - 1, 0):r + 2, max(cc - 1, 0):cc + 2] = 1
		mini.append(m)
	counts = np.diff(offs)
	assert counts.max() >= 4 and len(set(counts)) >= 3, counts
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps)))
	tx, ty = ctx.array(model.tx), ctx.array(model.ty)
	whole = engine.psf_fit(ctx, DeviceCube.from_host(ctx, s.images), DeviceCube.from_host(ctx, s.backgrounds), coef, tx, ty,
		ctx.array(np.asarray(offs, dtype='int64')), ctx.array(np.concatenate(params)), ctx.array(np.stack(mini)))
	whole = {k: whole[k].to_host() for k in ('flux', 'centroid_row', 'centroid_col', 'nit')}
	coef_h = coef.to_host()
	for i in range(0, Nt, 3):
		one = engine.psf_fit(ctx, DeviceCube.from_host(ctx, s.images[i:i + 1]), DeviceCube.from_host(ctx, s.backgrounds[i:i + 1]), ctx.array(coef_h[i:i + 1]), tx, ty,
			ctx.array(np.array([0, len(params[i])], dtype='int64')), ctx.array(params[i]), ctx.array(mini[i][None]))
		for k in ('flux', 'centroid_row', 'centroid_col', 'nit'):
			np.testing.assert_array_equal(one[k].to_host()[0][:T], whole[k][i][:T], err_msg=f'target {i} ({counts[i]} stars) {k}')


def test_psf_fit_is_reproducible(ctx):
	"""Two runs of the same batch give the same bits: iteration counts, fluxes, centroids.  (Until round 4 the thread that accepted a
	simplex point overwrote fsim[D] while slower wavefronts of the workgroup could still be comparing with it -- a spurious shrink
	step now and then, different from run to run: 256 targets x 6 cadences showed it in every run once the barrier that ended
	every likelihood evaluation was gone, and rarely before.)"""
	from photometry_amd import simulate, engine, psf as hpsf
	from photometry_amd.device import DeviceCube
	from photometry_amd.plugins import psf_star_selection, mag2flux
	Nt, T, H, W = 256, 6, 15, 15
	s = simulate.make_scene(Nt, T, H, W, seed=7)
	simulate.fill_cubes(s, nan_fraction=0.001)
	prf = simulate.synthetic_prf(seed=1)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	offs, params, mini = [0], [], []
	for i in range(Nt):
		c = s.catalog_of(i)
		sel = psf_star_selection(c['row_stamp'], c['column_stamp'], c['tmag'], s.target_pos_row[i] - s.stamps[i][0], s.target_pos_column[i] - s.stamps[i][2], s.target_tmag[i])
		params.append(np.column_stack((c['row_stamp'][sel].astype('float64'), c['column_stamp'][sel].astype('float64'), mag2flux(c['tmag'][sel].astype('float64')))))
		offs.append(offs[-1] + len(sel))
		m = np.zeros((H, W), dtype='uint8'); m[5:10, 5:10] = 1
		mini.append(m)
	assert len(set(np.diff(offs))) >= 3
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps)))
	args = (DeviceCube.from_host(ctx, s.images), DeviceCube.from_host(ctx, s.backgrounds), coef, ctx.array(model.tx), ctx.array(model.ty),
		ctx.array(np.asarray(offs, dtype='int64')), ctx.array(np.concatenate(params)), ctx.array(np.stack(mini)))
	runs = []
	for _ in range(3):
		r = engine.psf_fit(ctx, *args)
		runs.append({k: r[k].to_host()[:, :T].copy() for k in ('flux', 'centroid_row', 'centroid_col', 'nit')})
	for other in runs[1:]:
		for k in ('nit', 'flux', 'centroid_row', 'centroid_col'):
			np.testing.assert_array_equal(other[k], runs[0][k], err_msg=k)
