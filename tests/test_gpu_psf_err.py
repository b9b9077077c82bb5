# -*- coding: utf-8 -*-
"""
``tp_psf_flux_err`` / ``tp_psf_flux_err_xy`` through the C ABI against the CPU restatement of the definition
(``tests/psf_err_common.py``), to 1e-8 relative with the NaN pattern equal.  The parameters are given directly (the
oracle's synthetic truth plus offsets of a few hundredths of a pixel and a few per cent in flux): the definition holds at any theta,
no fit is needed.  The shapes are the smallest that can go wrong: stamps 11 x 11, 15 x 15 and 11 x 17 (121 .. 225 pixels over 64
lanes: two to four turns, the last one partial), 1, 2, 3 and 5 fitted stars and a catalogue of 6 (five are used) in one batch, 1, 3
and 65 cadences, padded pitches with a sentinel, NaN pixels / backgrounds / errors / parameters, a cadence without a good pixel, a
target without a star, a star at the stamp edge, no background cube, a rectangular and a warped PRF grid, no cut-off, a neighbour
of zero flux, an exactly singular normal matrix, reproducibility, batch independence, exact doubling, and the fit left untouched.
"""
import ctypes
import numpy as np
import pytest
import psf_err_common as pe

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _cube(ctx, cube, T, tp):
	from photometry_amd.device import DeviceCube
	if tp is None:
		return DeviceCube.from_host(ctx, np.ascontiguousarray(cube))
	n, H, W = cube.shape[:3]
	d = DeviceCube(ctx, n, T, H, W, t_pitch=tp)
	padded = np.full((n, H, W, tp), np.float32(SENTINEL))
	padded[..., :T] = cube
	d.data = ctx.array(padded)
	return d


def run_err(ctx, s, idx=None, pitches=None, backgrounds=True, xy=False, images_err=None, theta=None):
	"""The entry through the C ABI for the targets ``idx`` of a scene; returns the host ``(n, out_pitch)`` plane."""
	from photometry_amd import engine
	model = pe.host_model(s.kind)
	T = s.n_cad
	idx = np.arange(s.n_targets) if idx is None else np.asarray(idx)
	pp, op, tp = (T, T, None) if pitches is None else pitches
	thetas = [(s.theta if theta is None else theta)[i] for i in idx]
	plane, offs = pe.params_plane(thetas, T, pitch=pp, fill=SENTINEL)
	cubes = [_cube(ctx, c[idx], T, tp) for c in (s.images, s.backgrounds, s.images_err if images_err is None else images_err)]
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps[idx])))
	tx, ty = ctx.array(model.tx), ctx.array(model.ty)
	n, ny = len(model.tx) - 4, len(model.ty) - 4
	out = ctx.array(np.full((len(idx), op), SENTINEL))
	d_off, d_par, d_mini = ctx.array(offs), ctx.array(plane), ctx.array(np.ascontiguousarray(s.mini[idx]))
	desc = cubes[0].desc
	radius = float('inf') if s.cutoff_radius is None else float(s.cutoff_radius)
	bkg = cubes[1].ptr if backgrounds else None
	if xy:
		ctx._check(ctx.lib.tp_psf_flux_err_xy(ctx.handle, ctypes.byref(desc), cubes[0].ptr, bkg, cubes[2].ptr, coef.ptr, tx.ptr, ty.ptr, n, ny,
			d_off.ptr, d_par.ptr, pp, d_mini.ptr, pe.VAR_FLOOR, radius, out.ptr, op))
	else:
		assert n == ny
		ctx._check(ctx.lib.tp_psf_flux_err(ctx.handle, ctypes.byref(desc), cubes[0].ptr, bkg, cubes[2].ptr, coef.ptr, tx.ptr, ty.ptr, n,
			d_off.ptr, d_par.ptr, pp, d_mini.ptr, pe.VAR_FLOOR, radius, out.ptr, op))
	res = out.to_host()
	ctx.sync()
	for c in cubes:
		c.free()
	return res


def check(ctx, name, **kw):
	"""A parity scene on the device against its restatement."""
	s, rkw = pe.parity_scenes()[name]
	got = run_err(ctx, s, backgrounds=rkw.get('backgrounds', True), **kw)
	ref, _ = pe.parity_reference(name)
	worst = 0.0
	for i in range(s.n_targets):
		pe.assert_flux_err(got[i, :s.n_cad], ref[i], label=f'{name} target {i}')
		ok = np.isfinite(ref[i]) & (ref[i] != 0)
		if ok.any():
			worst = max(worst, float(np.max(np.abs(got[i, :s.n_cad][ok] / ref[i][ok] - 1))))
	print(f'{name}: worst relative difference device / restatement {worst:.2e}')
	return got, ref


# ---- star counts (1, 2, 3, 5 and a catalogue of 6) in one batch, stamp shapes ----
@pytest.mark.parametrize('H,W', [(11, 11), (15, 15), (11, 17)])
def test_star_counts(ctx, H, W):
	s, _ = pe.parity_scenes()[f'counts_{H}x{W}']
	assert [th.shape[1] for th in s.theta] == [1, 2, 3, 5, 6] and s.n_cad == 3
	got, ref = check(ctx, f'counts_{H}x{W}')
	assert np.all(np.isfinite(got)) and np.all(got > 0)
	# the sixth star of the catalogue is not used: dropping it from the parameters changes no bit
	theta5 = list(s.theta)
	theta5[4] = s.theta[4][:, :5, :]
	np.testing.assert_array_equal(run_err(ctx, s, theta=theta5), got)


@pytest.mark.parametrize('T', [1, 65])
def test_series_lengths(ctx, T):
	check(ctx, f'series_{T}')


# ---- layouts: every pitch larger than T, a sentinel beyond T that must survive ----
def test_pitches_and_sentinel(ctx):
	s, _ = pe.parity_scenes()['counts_11x11']
	T = s.n_cad
	got, _ = check(ctx, 'counts_11x11', pitches=(T + 3, T + 6, T + 5))
	assert got.shape == (5, T + 6) and np.all(got[:, T:] == SENTINEL)
	np.testing.assert_array_equal(got[:, :T], run_err(ctx, s)[:, :T])


# ---- data edges ----
def test_data_edges(ctx):
	got, ref = check(ctx, 'data_edges')
	for i in (0, 1):
		assert np.all(np.isfinite(got[i, [0, 3]])) and np.all(got[i, [0, 3]] > 0)
		assert np.isnan(got[i, 1]) and np.isnan(got[i, 2]) and np.isnan(got[i, 5])
		assert got[i, 4] == 0.0
	assert np.all(np.isnan(got[2]))      # nothing fitted


def test_star_at_the_stamp_edge(ctx):
	s, _ = pe.parity_scenes()['edge']
	assert s.truths[0][1, 1] < 0 and s.truths[1][0, 0] < 0.5      # within half a pixel of the edge (pixel centres start at 0)
	got, _ = check(ctx, 'edge')
	assert np.all(np.isfinite(got))


def test_no_background_cube(ctx):
	check(ctx, 'no_background')


# ---- any grid, any radius ----
def test_rectangular_grid_through_xy(ctx):
	m = pe.host_model('rect')
	assert len(m.tx) != len(m.ty)
	check(ctx, 'rect', xy=True)


def test_warped_knots(ctx):
	check(ctx, 'warped')


def test_no_cutoff(ctx):
	check(ctx, 'no_cutoff')


def test_zero_flux_neighbour(ctx):
	s, _ = pe.parity_scenes()['zero_flux']
	assert np.all(s.theta[0][:, 1, 2] == 0.0)
	got, _ = check(ctx, 'zero_flux')
	assert np.all(np.isfinite(got))


# ---- an exactly singular normal matrix: two neighbours at the same place with the same flux ----
def test_coincident_neighbours(ctx):
	truth = pe.stars_of(3, 11, 11)
	truth[2] = truth[1]
	s = pe.make_scene([truth, pe.stars_of(2, 11, 11)], 3, 11, 11, seed=130)
	s.theta[0][:, 2, :] = s.theta[0][:, 1, :]
	first = run_err(ctx, s)
	assert np.all(np.isfinite(first)) and np.all(first >= 0)
	np.testing.assert_array_equal(run_err(ctx, s), first)


# ---- reproducible, batch-independent, exact under doubling; the fit untouched ----
def test_bits(ctx):
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	s, _ = pe.parity_scenes()['counts_15x15']
	first = run_err(ctx, s)
	assert np.all(np.isfinite(first)) and np.all(first > 0)
	np.testing.assert_array_equal(run_err(ctx, s), first)                          # two calls
	for i in (0, 2, 4):                                                            # a target alone, another LDS size than in the batch
		np.testing.assert_array_equal(run_err(ctx, s, idx=[i])[0], first[i])
	np.testing.assert_array_equal(run_err(ctx, s, idx=[3, 1])[[1, 0]], first[[1, 3]])
	np.testing.assert_array_equal(run_err(ctx, s, images_err=s.images_err * np.float32(2)), 2.0 * first)   # err x 2
	# tp_psf_fit before and after the error pass: the same bits, flux_err still NaN
	model = pe.host_model(s.kind)
	idx = [0, 1, 2]
	plane, offs = pe.params_plane([s.truths[i][None] for i in idx], 1)

	def fit_once():
		coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps[idx])))
		images, backgrounds = DeviceCube.from_host(ctx, np.ascontiguousarray(s.images[idx])), DeviceCube.from_host(ctx, np.ascontiguousarray(s.backgrounds[idx]))
		r = engine.psf_fit(ctx, images, backgrounds, coef, ctx.array(model.tx), ctx.array(model.ty), ctx.array(offs),
			ctx.array(np.ascontiguousarray(plane[:, 0].reshape(-1, 3))), ctx.array(np.ascontiguousarray(s.mini[idx])))
		r = {k: v.to_host() for k, v in r.items()}
		ctx.sync()
		images.free()
		backgrounds.free()
		return r
	before = fit_once()
	np.testing.assert_array_equal(run_err(ctx, s), first)
	after = fit_once()
	for key in before:
		np.testing.assert_array_equal(before[key], after[key], err_msg=key)
	assert np.all(np.isnan(after['flux_err'])) and np.any(np.isfinite(after['flux']))


def test_engine_entry_on_the_fits_own_parameters(ctx):
	"""``engine.psf_flux_err`` on ``engine.psf_fit(...)['params']`` -- the layout the fit writes -- equals the restatement at those parameters."""
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	s, _ = pe.parity_scenes()['counts_11x11']
	model = pe.host_model(s.kind)
	idx, T = [0, 1, 2], s.n_cad
	plane, offs = pe.params_plane([s.truths[i][None] for i in idx], 1)
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps[idx])))
	cubes = [DeviceCube.from_host(ctx, np.ascontiguousarray(c[idx])) for c in (s.images, s.backgrounds, s.images_err)]
	tx, ty, d_off, d_mini = ctx.array(model.tx), ctx.array(model.ty), ctx.array(offs), ctx.array(np.ascontiguousarray(s.mini[idx]))
	fit = engine.psf_fit(ctx, cubes[0], cubes[1], coef, tx, ty, d_off, ctx.array(np.ascontiguousarray(plane[:, 0].reshape(-1, 3))), d_mini)
	got = engine.psf_flux_err(ctx, cubes[0], cubes[1], cubes[2], coef, tx, ty, d_off, fit['params'], d_mini).to_host()
	params, flux = fit['params'].to_host(), fit['flux'].to_host()
	ctx.sync()
	for c in cubes:
		c.free()
	assert got.shape == (3, T)
	for j, i in enumerate(idx):
		S = int(offs[j + 1] - offs[j])
		theta = params[3 * offs[j]:3 * offs[j + 1], :T].T.reshape(T, S, 3)
		ref = pe.flux_err_series(pe.oracle_psf(s.kind, s.stamps[i]), s.images[i], s.backgrounds[i], s.images_err[i], theta, s.mini[i])
		np.testing.assert_array_equal(np.isnan(ref), np.isnan(flux[j, :T]))      # NaN exactly where the fit did not finish
		pe.assert_flux_err(got[j], ref, label=f'engine target {i}')
	assert np.any(np.isfinite(got))
