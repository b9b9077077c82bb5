# -*- coding: utf-8 -*-
"""
``tp_linpsf_flux_err`` / ``tp_linpsf_flux_err_xy`` through the C ABI against the CPU restatement of the definition
(``tests/linpsf_err_common.py``), to 1e-8 relative -- the project's LinPSF tolerance -- with the NaN pattern equal.
Scenes are designed (``linpsf_common.design_target``): stars separated as in the fit's class tests.  The shapes are the smallest
that can go wrong: every star-count class and its borders (1, 2 | 3, 4 | 5, 8 | 9, 12), the target anywhere in its list, series
of 1 / 63 / 65 cadences and one beyond a workgroup (259: the kernel's workgroup is 256 lanes), square and rectangular stamps,
padded pitches, NaN pixels and errors, stars at the stamp edge, a non-SPOC and a rectangular PRF grid, no cut-off, a singular
normal matrix, reproducibility, batch independence, exact scaling, and the fit left untouched.
"""
import ctypes
import numpy as np
import pytest
import linpsf_common as lc
import linpsf_err_common as le

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _scene(specs, T, H, W, seed, **kw):
	s = le.add_errors(lc.designed_scene(specs, T, H, W, seed=seed, **kw))
	_, so, ti, pr, pc = lc.fit_inputs(s)
	return s, (so, ti, pr, pc)


def _subset(fit, idx):
	so, ti, pr, pc = fit
	stars = np.concatenate([np.arange(so[i], so[i + 1]) for i in idx])
	offs = np.concatenate(([0], np.cumsum([so[i + 1] - so[i] for i in idx]))).astype('int64')
	return offs, np.ascontiguousarray(ti[idx]), np.ascontiguousarray(pr[stars]), np.ascontiguousarray(pc[stars])


def _padded_cube(ctx, cube, T, tp):
	from photometry_amd.device import DeviceCube
	n, H, W = cube.shape[:3]
	d = DeviceCube(ctx, n, T, H, W, t_pitch=tp)
	padded = np.full((n, H, W, tp), np.float32(SENTINEL))
	padded[..., :T] = cube
	d.data = ctx.array(padded)
	return d


def run_err(ctx, s, fit, kind='spoc', idx=None, cutoff=5, pitches=None, images=None, images_err=None, xy=False):
	"""The entry through the C ABI for the targets ``idx`` of a scene; returns the host ``(n, out_pitch)`` plane."""
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	_, model = lc.prf_and_model(kind)
	T = s.n_cad
	idx = np.arange(s.n_targets) if idx is None else np.asarray(idx)
	offs, ti, pr, pc = _subset(fit, idx)
	images = (s.images if images is None else images)[idx]
	images_err = (s.images_err if images_err is None else images_err)[idx]
	pp, op, tp = (T, T, None) if pitches is None else pitches
	if pp > T:
		prp, pcp = np.full((len(pr), pp), SENTINEL), np.full((len(pr), pp), SENTINEL)
		prp[:, :T], pcp[:, :T] = pr, pc
		pr, pc = prp, pcp
	if tp is None:
		cube, ecube = DeviceCube.from_host(ctx, np.ascontiguousarray(images)), DeviceCube.from_host(ctx, np.ascontiguousarray(images_err))
	else:
		cube, ecube = _padded_cube(ctx, images, T, tp), _padded_cube(ctx, images_err, T, tp)
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps[idx])))
	tx, ty = ctx.array(model.tx), ctx.array(model.ty)
	n, ny = len(model.tx) - 4, len(model.ty) - 4
	out = ctx.array(np.full((len(idx), op), SENTINEL))
	d_off, d_ti, d_pr, d_pc = ctx.array(offs), ctx.array(ti), ctx.array(pr), ctx.array(pc)
	desc = cube.desc
	radius = float('inf') if cutoff is None else float(cutoff)
	max_stars = max(int(np.diff(offs).max()), 1)
	if xy:
		ctx._check(ctx.lib.tp_linpsf_flux_err_xy(ctx.handle, ctypes.byref(desc), cube.ptr, ecube.ptr, coef.ptr, tx.ptr, ty.ptr, n, ny, max_stars,
			d_off.ptr, d_ti.ptr, d_pr.ptr, d_pc.ptr, pr.shape[1], radius, out.ptr, op))
	else:
		assert n == ny
		ctx._check(ctx.lib.tp_linpsf_flux_err(ctx.handle, ctypes.byref(desc), cube.ptr, ecube.ptr, coef.ptr, tx.ptr, ty.ptr, n, max_stars,
			d_off.ptr, d_ti.ptr, d_pr.ptr, d_pc.ptr, pr.shape[1], radius, out.ptr, op))
	res = out.to_host()
	ctx.sync()
	cube.free()
	ecube.free()
	return res


def check(ctx, s, fit, kind='spoc', cutoff=5, rtol=1e-8, label='', **kw):
	got = run_err(ctx, s, fit, kind=kind, cutoff=cutoff, **kw)
	T = s.n_cad
	for i in range(s.n_targets):
		ref = le.restate_target(s, fit, i, kind=kind, cutoff_radius=cutoff, images=kw.get('images'), images_err=kw.get('images_err'))
		le.assert_flux_err(got[i, :T], ref, rtol=rtol, label=f'{label} target {i}')
	return got


def _model():
	return lc.prf_and_model('spoc')[1]


# ---- star-count classes, the target anywhere in its list, stamp shapes ----
@pytest.mark.parametrize('H,W', [(11, 11), (15, 15), (11, 17)])
def test_star_counts(ctx, H, W):
	T = 3
	m = _model()
	places = {1: 0, 2: 1, 3: 0, 4: 3, 5: 2, 8: 7, 9: 4, 12: 11}
	specs = [lc.design_target(m, S, places[S], T, H, W, shape=(2, 1), seed=300 + S, layout='disc' if S > 8 else 'ring') for S in (1, 2, 3, 4, 5, 8, 9, 12)]
	s, fit = _scene(specs, T, H, W, seed=11)
	assert list(np.diff(fit[0])) == [1, 2, 3, 4, 5, 8, 9, 12]
	check(ctx, s, fit, label=f'{H}x{W}')


def test_target_at_every_place(ctx):
	T, H, W = 2, 11, 11
	m = _model()
	s, fit = _scene([lc.design_target(m, 4, place, T, H, W, seed=310 + place) for place in range(4)], T, H, W, seed=12)
	assert list(fit[1]) == [0, 1, 2, 3]
	check(ctx, s, fit, label='places')


# ---- series lengths: one cadence, either side of a wavefront, more than one workgroup ----
@pytest.mark.parametrize('T', [1, 63, 65])
def test_series_lengths(ctx, T):
	H = W = 11
	m = _model()
	s, fit = _scene([lc.design_target(m, 1, 0, T, H, W, seed=320), lc.design_target(m, 3, 2, T, H, W, seed=321)], T, H, W, seed=13)
	check(ctx, s, fit, label=f'T={T}')


def test_more_cadences_than_a_workgroup(ctx):
	T, H, W = 259, 11, 11
	m = _model()
	s, fit = _scene([lc.design_target(m, 1, 0, T, H, W, seed=330)], T, H, W, seed=14)
	check(ctx, s, fit, label='T=259')


# ---- layouts: padded pitches with a sentinel beyond n_cad, on the register classes and the workspace kernel ----
def test_pitches_and_sentinel(ctx):
	T, H, W = 5, 11, 11
	m = _model()
	s, fit = _scene([lc.design_target(m, 2, 1, T, H, W, seed=340), lc.design_target(m, 9, 3, T, H, W, seed=341, layout='disc')], T, H, W, seed=15)
	got = check(ctx, s, fit, pitches=(T + 3, T + 6, T + 11), label='pitches')
	assert got.shape == (2, T + 6) and np.all(got[:, T:] == SENTINEL)


# ---- data edges ----
def test_nan_pixels_nan_errors_and_an_empty_cadence(ctx):
	T, H, W = 6, 11, 11
	m = _model()
	s, fit = _scene([lc.design_target(m, 1, 0, T, H, W, seed=350), lc.design_target(m, 3, 1, T, H, W, seed=351),
		lc.design_target(m, 10, 2, T, H, W, seed=352, layout='disc')], T, H, W, seed=16, nan_fraction=0.004)
	assert np.isnan(s.images).any()
	images, err = s.images.copy(), s.images_err.copy()
	images[:, :, :, 4] = np.nan                 # a cadence without a good pixel -> 0
	for i in range(3):
		good = np.argwhere(np.isfinite(images[i][:, :, 1]))
		r, c = good[0]                          # the first good pixel: a corner region, outside the single star's cut-off disc
		err[i, r, c, 1] = np.nan                # a NaN err at a good pixel -> NaN there only
		r, c = good[len(good) // 2]
		err[i, r, c, 2] = np.inf
	bad = ~np.isfinite(images)
	err[bad] = np.where(np.arange(bad.sum()) % 2 == 0, np.float32(np.nan), np.float32(3.0))   # anything where the image is not finite: no effect
	got = check(ctx, s, fit, images=images, images_err=err, label='nan')
	assert np.all(got[:, 4] == 0.0) and np.all(np.isnan(got[:, 1])) and np.all(np.isnan(got[:, 2]))
	assert np.all(np.isfinite(got[:, [0, 3, 5]]))


def test_stars_at_the_stamp_edge(ctx):
	T, H, W = 3, 11, 11
	m = _model()
	# the neighbour 0.2 px inside the left edge of the stamp (pixel centres start at 0: the edge is at -0.5); the second target's
	# neighbour sits in the corner region, most of its cut-off circle outside the stamp
	s, fit = _scene([lc.design_target(m, 2, 0, T, H, W, positions=[(5.2, 4.1), (5.9, -0.3)], motion=np.zeros((T, 2)), seed=360),
		lc.design_target(m, 2, 1, T, H, W, positions=[(1.6, 8.4), (4.8, 5.3)], motion=np.zeros((T, 2)), seed=361)], T, H, W, seed=17)
	assert fit[3][1].max() < -0.2 and list(np.diff(fit[0])) == [2, 2]
	check(ctx, s, fit, label='edge')


# ---- any grid, any radius ----
def test_non_spoc_grid(ctx):
	T, H, W = 2, 13, 13
	m = _model()
	s, fit = _scene(lc._targets_anygrid(m, T, H, W), T, H, W, seed=18)
	check(ctx, s, fit, kind='warped', label='warped grid')


def test_rectangular_grid_through_xy(ctx):
	T, H, W = 2, 13, 13
	m = _model()
	s, fit = _scene(lc._targets_anygrid(m, T, H, W)[:2], T, H, W, seed=19)
	check(ctx, s, fit, kind='rect', xy=True, label='rect grid')


def test_no_cutoff(ctx):
	T, H, W = 2, 13, 13
	m = _model()
	s, fit = _scene(lc._targets_anygrid(m, T, H, W)[:2], T, H, W, seed=20)
	check(ctx, s, fit, cutoff=None, label='no cut-off')


# ---- singular normal matrix: two fitted stars at exactly the same place ----
def test_coincident_stars(ctx):
	T, H, W = 3, 11, 11
	m = _model()
	specs = [lc.design_target(m, 2, 0, T, H, W, positions=[(5.2, 4.9), (5.2, 4.9)], motion=np.zeros((T, 2)), seed=370),
		lc.design_target(m, 2, 1, T, H, W, positions=[(4.7, 5.4), (4.7, 5.4)], motion=np.zeros((T, 2)), seed=371)]
	s, fit = _scene(specs, T, H, W, seed=21)
	assert np.array_equal(fit[2][0], fit[2][1]) and np.array_equal(fit[3][2], fit[3][3])
	got = check(ctx, s, fit, label='coincident')
	assert np.all(np.isfinite(got)) and np.all(got > 0)


# ---- reproducible, batch-independent, exact under scaling; the fit untouched ----
def test_bits(ctx):
	from photometry_amd import engine
	from photometry_amd.device import DeviceCube
	T, H, W = 9, 11, 11
	m = _model()
	counts = [(1, 0), (3, 1), (6, 5), (2, 1), (9, 8), (4, 0)]
	s, fit = _scene([lc.design_target(m, S, place, T, H, W, seed=380 + q, layout='disc' if S > 8 else 'ring') for q, (S, place) in enumerate(counts)], T, H, W, seed=22)
	first = run_err(ctx, s, fit)
	assert np.all(np.isfinite(first)) and np.all(first > 0)
	np.testing.assert_array_equal(run_err(ctx, s, fit), first)                      # two calls
	for i in (3, 4):                                                               # a target alone
		np.testing.assert_array_equal(run_err(ctx, s, fit, idx=[i])[0], first[i])
	np.testing.assert_array_equal(run_err(ctx, s, fit, images_err=s.images_err * np.float32(2)), 2.0 * first)   # err x 2
	# tp_linpsf_fit before and after the error pass: the same bits, flux_err still NaN
	_, model = lc.prf_and_model('spoc')
	so, ti, pr, pc = fit

	def fit_once():
		cube = DeviceCube.from_host(ctx, s.images)
		coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps)))
		r = engine.linpsf_fit(ctx, cube, coef, ctx.array(model.tx), ctx.array(model.ty), ctx.array(so), ctx.array(ti), ctx.array(pr), ctx.array(pc),
			int(np.diff(so).max())).to_host()
		cube.free()
		return r
	before = fit_once()
	np.testing.assert_array_equal(run_err(ctx, s, fit), first)
	after = fit_once()
	for key in before:
		np.testing.assert_array_equal(before[key], after[key], err_msg=key)
	assert np.all(np.isnan(after['flux_err']))
