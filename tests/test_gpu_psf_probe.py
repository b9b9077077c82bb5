# -*- coding: utf-8 -*-
"""
The pixel model and the warm-start chain of ``tp_psf_fit`` / ``tp_psf_fit_xy`` against the oracle value for value, without a
Nelder-Mead walk having to agree (``tests/psf_probe_common.py``; the premises are pinned on the CPU by ``test_psf_probe_host.py``).

A cadence whose weights are all NaN has a constant objective: the fit ends with ``success`` at its start point ``x0`` bit for bit after
the oracle walk's iteration count, and with a one-pixel mini aperture over a zero image ``flux`` is ``f0 - model_p(x0)`` -- the
kernel's model of one pixel, in the instantiation under test (1 .. 5 fitted stars, cached or general), with the cached sets and the
store in the state the shrink walk left them.  It is held to ``oracle.psf.PSF.integrate_to_image`` at ``BOUND`` = 100 x ``FLOOR`` =
2e-13 of the peak.  On real fits two identities need no walk to agree either: ``flux[k]`` is ``params_out[2][k]`` plus the residuals
of the oracle's model at the device's own end point, and a constant-objective cadence ends exactly at the last finished cadence's
parameters.  Every call runs with the per-target store of built sets and with ``TESSPHOT_PSF_STORE=0``: the same bits in every output.

Measured on an MI355X (worst ``|device - oracle| / peak + 2^-53 f0 / peak`` over all probe calls; ``test_report_worst`` prints them):
cached path 1.01e-14 (9.2e-15 of it is the biquartic form itself, test_psf_probe_host.py), general path 1.24e-15, cached against
general on the same point 7.6e-15, the aperture-correction identity on real fits 7.9e-15 per mini-aperture pixel; the bound is 2e-13.
Every probe fit took the oracle walk's 25 iterations (31 with a star at 2e6).
"""
import ctypes
import numpy as np
import pytest
import psf_err_common as pe
import psf_probe_common as pc

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
TP_STATUS_OK, TP_STATUS_ERROR = 1, 2
OUT_KEYS = ('flux', 'flux_err', 'centroid_row', 'centroid_col', 'params', 'nit', 'status')

_worst = {'cached': 0.0, 'general': 0.0, 'identity': 0.0}


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _cube(ctx, cube, tp):
	"""A device cube of pitch ``tp`` whose padding holds the byte pattern."""
	from photometry_amd.device import DeviceCube
	n, H, W, T = cube.shape
	d = DeviceCube(ctx, n, T, H, W, t_pitch=tp)
	padded = np.frombuffer(bytes([PATTERN]) * (n * H * W * tp * 4), dtype='float32').reshape(n, H, W, tp).copy()
	padded[..., :T] = cube
	d.data = ctx.array(padded)
	return d


def _patterned(ctx, shape, dtype):
	a = ctx.empty(shape, dtype)
	a.fill_bytes(PATTERN)
	return a


def is_pattern(a):
	return np.all(np.ascontiguousarray(a).view('uint8') == PATTERN)


def fit(ctx, monkeypatch, model, stamps, images, backgrounds, star_offsets, params0, mini, radius, t_pitch=32, out_pitch=None, var_floor=pe.VAR_FLOOR,
		maxiter=(1500, 500), xy=False):
	"""``tp_psf_fit`` (``xy``: ``tp_psf_fit_xy``) through the C ABI on outputs prefilled with the byte pattern, once with the store and once
	with ``TESSPHOT_PSF_STORE=0``: every output agrees bit for bit; returns the host arrays (``params`` ``(n_stars * 3, out_pitch)``)."""
	from photometry_amd import engine
	n, H, W, T = images.shape
	op = T + 2 if out_pitch is None else out_pitch
	n_stars = max(int(star_offsets[-1]), 1)
	coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(stamps)))
	d_img = _cube(ctx, images, t_pitch)
	d_bkg = None if backgrounds is None else _cube(ctx, backgrounds, t_pitch)
	tx, ty = ctx.array(model.tx), ctx.array(model.ty)
	d_off, d_par, d_mini = ctx.array(np.asarray(star_offsets, dtype='int64')), ctx.array(np.ascontiguousarray(params0, dtype='float64').reshape(-1, 3) if len(params0) else np.zeros((1, 3))), ctx.array(np.ascontiguousarray(mini, dtype='uint8'))
	desc = d_img.desc
	runs = []
	for store in (None, '0'):
		if store is None:
			monkeypatch.delenv('TESSPHOT_PSF_STORE', raising=False)
		else:
			monkeypatch.setenv('TESSPHOT_PSF_STORE', store)
		out = {k: _patterned(ctx, (n, op), 'float64') for k in OUT_KEYS[:4]}
		out['params'] = _patterned(ctx, (n_stars * 3, op), 'float64')
		out['nit'] = _patterned(ctx, (n, op), 'int32')
		out['status'] = _patterned(ctx, (n,), 'int32')
		tail = (d_off.ptr, d_par.ptr, d_mini.ptr, float(var_floor), float(radius), int(maxiter[0]), int(maxiter[1]), out['flux'].ptr, out['flux_err'].ptr,
			out['centroid_row'].ptr, out['centroid_col'].ptr, op, out['params'].ptr, out['nit'].ptr, out['status'].ptr)
		head = (ctx.handle, ctypes.byref(desc), d_img.ptr, None if d_bkg is None else d_bkg.ptr, coef.ptr, tx.ptr, ty.ptr)
		if xy:
			ctx._check(ctx.lib.tp_psf_fit_xy(*head, len(model.tx) - 4, len(model.ty) - 4, *tail))
		else:
			assert len(model.tx) == len(model.ty)
			ctx._check(ctx.lib.tp_psf_fit(*head, len(model.tx) - 4, *tail))
		runs.append({k: out[k].to_host() for k in OUT_KEYS})
		ctx.sync()
	monkeypatch.delenv('TESSPHOT_PSF_STORE', raising=False)
	for k in OUT_KEYS:
		assert runs[0][k].tobytes() == runs[1][k].tobytes(), f'{k}: the store changes bits'
	d_img.free()
	if d_bkg is not None:
		d_bkg.free()
	res = runs[0]
	for k in OUT_KEYS[:6]:
		assert is_pattern(res[k][:, T:]), f'{k}: written beyond n_cad'
	return res


def run_probe(ctx, monkeypatch, name, T=2, path=None, nan_background=True, **kw):
	"""One probe call against its reference; returns ``(res, inputs, worst error measure)``."""
	probes = pc.probe_points()[name]
	ref = pc.reference(name)
	a = pc.probe_inputs(probes, T=T, nan_background=nan_background)
	model = pe.host_model(probes[0].kind)
	if not nan_background:
		kw['var_floor'] = float('nan')
	res = fit(ctx, monkeypatch, model, a['stamps'], a['images'], a['backgrounds'], a['star_offsets'], a['params0'], a['mini'], probes[0].radius, **kw)
	worst = 0.0
	t = 0
	for q, p in enumerate(probes):
		expect, peak, nit = ref[q]
		sl = slice(t, t + len(p.pixels))
		t += len(p.pixels)
		S = len(p.fitted)
		if S == 0:
			# nothing to fit: every light-curve value NaN, the status an error
			for k in OUT_KEYS[:4]:
				assert np.all(np.isnan(res[k][sl, :T])), (name, q, k)
			assert np.all(res['status'][sl] == TP_STATUS_ERROR)
			continue
		assert np.all(res['status'][sl] == TP_STATUS_OK), (name, q)
		assert np.all(res['nit'][sl, :T] == nit), (name, q, nit, np.unique(res['nit'][sl, :T]))
		x0 = p.fitted.ravel()
		for k in range(T):
			assert res['centroid_row'][sl, k].tobytes() == np.full(len(p.pixels), x0[0]).tobytes(), (name, q, k)
			assert res['centroid_col'][sl, k].tobytes() == np.full(len(p.pixels), x0[1]).tobytes(), (name, q, k)
		assert np.all(np.isnan(res['flux_err'][sl, :T]))
		for u in range(len(p.pixels)):
			r0 = 3 * int(a['star_offsets'][sl.start + u])
			rows = res['params'][r0:r0 + 3 * len(p.x0), :T]
			assert rows[:3 * S].tobytes() == np.repeat(x0[:, None], T, axis=1).tobytes(), (name, q, u)      # the end point is the start point
			assert is_pattern(rows[3 * S:]), (name, q, u)                                                     # a sixth listed star is not fitted
		flux = res['flux'][sl, :T]
		assert np.all(flux == flux[:, :1]), (name, q)          # every cadence starts from x0 again: the same bits
		if peak == 0.0:
			assert np.all(flux == p.fitted[0, 2]), (name, q)   # no pixel inside any disc: the model is 0, exactly
			continue
		err = pc.model_error(flux[:, 0], p, expect)
		worst = max(worst, float(err.max()))
		assert err.max() <= pc.BOUND, (name, q, float(err.max()), int(p.pixels[err.argmax()]))
		zero = expect.ravel()[p.pixels] == 0.0
		assert np.all(flux[zero, 0] == p.fitted[0, 2]), (name, q)      # outside every cut-off: exactly f0
	assert t == len(a['owner'])
	path = path or ('cached' if (probes[0].kind == 'spoc' and probes[0].radius <= 5.25) else 'general')
	_worst[path] = max(_worst[path], worst)
	print(f'{name}: {t} targets, worst error measure {worst:.2e} of the peak ({path} path; bound {pc.BOUND:.0e})')
	return res, a, worst


# ---- every instantiation: 1 .. 5 fitted stars, cached and general; the walk crosses more sets than the store keeps ----
@pytest.mark.parametrize('S', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('kind', ['spoc', 'warped'])
def test_every_instantiation(ctx, monkeypatch, kind, S):
	run_probe(ctx, monkeypatch, f'inst_{kind}_{S}')


def test_mixed_batch(ctx, monkeypatch):
	"""Targets with 0, 1, 3, 5 and 6 listed stars in one call: three launches and the star-less class; of six stars five are fitted."""
	res, a, _ = run_probe(ctx, monkeypatch, 'mixed')
	probes = pc.probe_points()['mixed']
	five, six = (res['flux'][a['owner'] == q, :2] for q in (3, 4))
	assert five.tobytes() == six.tobytes() and len(probes[4].x0) == 6     # the sixth star changes no bit


def test_two_stars_in_the_same_intervals(ctx, monkeypatch):
	"""Two stars that need the set of the same pair of knot intervals in one evaluation, and keep it through the whole walk: each gets
	a built set, none a store slot that the other has only tagged.  (The store holds other sets from the call before.)"""
	run_probe(ctx, monkeypatch, 'inst_spoc_2')
	run_probe(ctx, monkeypatch, 'same_intervals')


# ---- the pixel loop ----
@pytest.mark.parametrize('name', ['stamp_17x17', 'stamp_5x23', 'stamp_3x3'])
def test_stamp_shapes(ctx, monkeypatch, name):
	run_probe(ctx, monkeypatch, name)


# ---- phases ----
@pytest.mark.parametrize('name', ['phase_sweep', 'phase_knots', 'outside_4p9', 'outside_5p1', 'invalid_star', 'invalid_star_general'])
def test_phases_and_positions(ctx, monkeypatch, name):
	res, a, _ = run_probe(ctx, monkeypatch, name)
	if name == 'outside_5p1':
		assert np.all(res['flux'][:, :2] == 30000.0)
	if name.startswith('invalid_star'):
		# the stars at 2e6 contribute nothing: the target's star alone gives the same bits
		(p,) = pc.probe_points()[name]
		alone = pc.Probe(p.kind, p.cutoff, p.H, p.W, p.x0[:1])
		b = pc.probe_inputs([alone], T=2)
		one = fit(ctx, monkeypatch, pe.host_model(p.kind), b['stamps'], b['images'], b['backgrounds'], b['star_offsets'], b['params0'], b['mini'], p.radius)
		assert one['flux'][:, :2].tobytes() == res['flux'][:, :2].tobytes()


# ---- the cut-off ----
def test_cutoff_is_strict(ctx, monkeypatch):
	res, a, _ = run_probe(ctx, monkeypatch, 'cutoff_integer')
	flux = res['flux'][:, 0].reshape(11, 11)
	for (i, j) in ((8, 9), (9, 8), (10, 5), (5, 0), (5, 10), (0, 5), (2, 1), (1, 2)):      # distance exactly 5: excluded (psf.py:142, `<`)
		assert flux[i, j] == 30000.0, (i, j)
	assert flux[9, 7] < 30000.0 and flux[5, 1] < 30000.0                                    # distance sqrt(20), 4: inside


@pytest.mark.parametrize('name', ['cutoff_5p25', 'cutoff_5p26', 'cutoff_none'])
def test_cutoff_radii(ctx, monkeypatch, name):
	"""5.25 is the largest radius of the cached path (the trimmed corner items of the 109-item set at phases +-0.499); 5.26 and no
	cut-off on the same grid take the general path."""
	run_probe(ctx, monkeypatch, name)


def test_cached_and_general_agree(ctx, monkeypatch):
	"""The same point on both paths (cut-off 5 cached, 5.26 general): where the two discs hold the same stars the values agree within the
	bound -- each is held to the oracle on its own by run_probe."""
	c, _, _ = run_probe(ctx, monkeypatch, 'paths_cached')
	g, _, _ = run_probe(ctx, monkeypatch, 'paths_general')
	(pc5,), (pg,) = pc.probe_points()['paths_cached'], pc.probe_points()['paths_general']
	same = (pc.reference('paths_cached')[0][0] == pc.reference('paths_general')[0][0]).ravel()
	assert same.sum() >= 100
	d = np.abs(c['flux'][same, 0] - g['flux'][same, 0]) / pc.peak_of(pc5)
	print(f'cached against general on {int(same.sum())} pixels: at most {d.max():.2e} of the peak')
	assert d.max() <= pc.BOUND


# ---- grids through tp_psf_fit_xy ----
@pytest.mark.parametrize('name', ['grid_rect', 'grid_nsub7', 'grid_coarse'])
def test_grids_through_xy(ctx, monkeypatch, name):
	m = pe.host_model(pc.probe_points()[name][0].kind)
	assert (len(m.tx) != len(m.ty)) == (name == 'grid_rect')
	run_probe(ctx, monkeypatch, name, xy=True)


# ---- layouts ----
def test_layouts(ctx, monkeypatch):
	"""Pitches beyond the cadences, one cadence, and no background cube under a NaN variance floor: the same bits as the NaN
	background gives."""
	base, _, _ = run_probe(ctx, monkeypatch, 'layout', T=2)
	for (T, tp, op) in ((1, 1, 1), (1, 4, 3), (2, 7, 5), (3, 3, 9)):
		res, _, _ = run_probe(ctx, monkeypatch, 'layout', T=T, t_pitch=tp, out_pitch=op)
		nul, _, _ = run_probe(ctx, monkeypatch, 'layout', T=T, t_pitch=tp, out_pitch=op, nan_background=False)
		for k in OUT_KEYS:
			assert res[k].tobytes() == nul[k].tobytes(), (T, tp, op, k)
		assert res['flux'][:, 0].tobytes() == base['flux'][:, 0].tobytes() and res['nit'][:, 0].tobytes() == base['nit'][:, 0].tobytes()


# --------------------------------------------------------------------------------------------------
# real fits: the aperture-correction identity and the chain
# --------------------------------------------------------------------------------------------------
def scene_inputs(s):
	"""Star lists, start parameters and mini apertures of a simulated scene, as the plugin forms them."""
	from photometry_amd.plugins import psf_star_selection, mag2flux
	from oracle.aperture import minimum_aperture
	offs, params, mini = [0], [], []
	for i in range(s.n_targets):
		c = s.catalog_of(i)
		sel = psf_star_selection(c['row_stamp'], c['column_stamp'], c['tmag'], s.target_pos_row[i] - s.stamps[i][0], s.target_pos_column[i] - s.stamps[i][2], s.target_tmag[i])
		params.append(np.column_stack((c['row_stamp'][sel].astype('float64'), c['column_stamp'][sel].astype('float64'), mag2flux(c['tmag'][sel].astype('float64')))))
		offs.append(offs[-1] + len(sel))
		mini.append(minimum_aperture(tuple(s.stamps[i]), s.target_pos_row[i], s.target_pos_column[i], s.aperture[i]))
	return np.asarray(offs, dtype='int64'), np.concatenate(params), np.stack(mini).astype('uint8')


def theta_of(res, offs, i, k):
	S = min(int(offs[i + 1] - offs[i]), pc.MAX_STARS)
	return res['params'][3 * offs[i]:3 * offs[i] + 3 * S, k].copy()


def identity_error(psf, img, mini, theta, flux, cutoff):
	"""``flux`` against ``f0 + nansum_mini(img - oracle model at theta)``: the error measure, relative to the peak, and the number of
	mini-aperture pixels the bound is multiplied by."""
	theta = theta.reshape(-1, 3)
	mdl = psf.integrate_to_image(theta.copy(), cutoff_radius=cutoff)
	peak = float(sum(abs(f) * np.max(psf.integrate_to_image(np.array([[r, c, 1.0]]), cutoff_radius=cutoff)) for (r, c, f) in theta))
	want = theta[0, 2] + np.nansum((img.astype('float64') - mdl)[mini.astype(bool)])
	return abs(flux - want) / peak + 2.0**-53 * abs(theta[0, 2]) / peak, max(int(mini.sum()), 1)


def check_identity(res, images, psf_of, offs, mini, cutoff, targets, label):
	"""The identity on every finished cadence of ``targets``; returns how many were checked."""
	T = images.shape[3]
	n = 0
	for i in targets:
		psf = psf_of(i)
		for k in range(T):
			theta = theta_of(res, offs, i, k)
			finished = not np.isnan(res['flux'][i, k])
			assert finished == bool(np.all(np.isfinite(theta))), (label, i, k)
			if not finished:
				continue
			assert res['centroid_row'][i, k] == theta[0] and res['centroid_col'][i, k] == theta[1]
			err, npx = identity_error(psf, images[i, :, :, k], mini[i], theta, res['flux'][i, k], cutoff)
			_worst['identity'] = max(_worst['identity'], err / npx)
			assert err <= pc.BOUND * npx, (label, i, k, err, npx)
			n += 1
	print(f'{label}: the aperture-correction identity on {n} finished cadences; worst so far {_worst["identity"]:.2e} of the peak per pixel')
	return n


def test_chain(ctx, monkeypatch):
	"""Four cadences of the real scene of test_psf_photometry_matches_oracle (its own lists of two to four stars, and each target again
	with one and with two): 0 and 1 ordinary, 2 with a constant objective -- it ends
	exactly at the last finished cadence's parameters -- and 3 ordinary but stopped by ``maxiter = 3`` in a second call that starts from
	the first call's cadence-2 parameters: ``nit == maxiter``, all-NaN outputs, and the constant-objective cadence after it still ends at
	that start.  Every finished cadence satisfies the aperture-correction identity at the device's own end point."""
	from photometry_amd import simulate, psf as hpsf
	from oracle import psf as opsf
	Nt, T, H, W = 5, 4, 11, 11
	s = simulate.make_scene(Nt, T, H, W, seed=91, max_neighbours=3, neighbour_tmag_range=(9.0, 15.0))
	simulate.fill_cubes(s, nan_fraction=0.004)
	prf = opsf.synthetic_prf(seed=5)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	offs, params0, mini = scene_inputs(s)
	# the scene's own star lists (two to four stars), and every target once more with its list cut to one and to two stars
	lists = [params0[offs[i]:offs[i + 1]] for i in range(Nt)]
	lists = lists + [p[:1] for p in lists] + [p[:2] for p in lists]
	idx = np.tile(np.arange(Nt), 3)
	Nt = len(idx)
	offs, params0 = np.concatenate(([0], np.cumsum([len(p) for p in lists]))).astype('int64'), np.concatenate(lists)
	counts = np.diff(offs)
	assert {1, 2} < set(counts.tolist()), counts
	images, stamps, mini = s.images[idx], s.stamps[idx], mini[idx]
	bkg = s.backgrounds[idx].copy()
	bkg[:, :, :, 2] = np.nan
	first = fit(ctx, monkeypatch, model, stamps, images[..., :3], bkg[..., :3], offs, params0, mini, 5.0)
	assert np.all(first['status'] == TP_STATUS_OK)

	def psf_of(i):
		return opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(stamps[i]))
	assert check_identity(first, images[..., :3], psf_of, offs, mini, 5, range(Nt), 'chain') > Nt      # cadence 2 always finishes; some ordinary ones do
	starts = []
	for i in range(Nt):
		fin = [k for k in (0, 1) if not np.isnan(first['flux'][i, k])]
		last = theta_of(first, offs, i, fin[-1]) if fin else params0[offs[i]:offs[i + 1]].ravel()
		got = theta_of(first, offs, i, 2)
		assert got.tobytes() == last.tobytes(), (i, fin)
		assert int(first['nit'][i, 2]) == pc.constant_walk(last, 500)[2], i
		for k in (0, 1):
			assert (k in fin) == (int(first['nit'][i, k]) < (1500 if k == 0 else 500)), (i, k)
		starts.append(got.reshape(-1, 3))
	print('chain: iterations', first['nit'][:, :3].tolist())
	# the second call: cadence 3 stopped after three iterations, then the constant-objective cadence once more
	images2 = np.stack((images[..., 3], images[..., 2]), axis=-1)
	bkg2 = np.stack((s.backgrounds[idx][..., 3], bkg[..., 2]), axis=-1)
	second = fit(ctx, monkeypatch, model, stamps, images2, bkg2, offs, np.concatenate(starts), mini, 5.0, maxiter=(3, 500))
	assert np.all(second['status'] == TP_STATUS_OK)
	for i in range(Nt):
		assert int(second['nit'][i, 0]) == 3
		for k in OUT_KEYS[:4]:
			assert np.isnan(second[k][i, 0]), (i, k)
		assert np.all(np.isnan(theta_of(second, offs, i, 0)))
		assert theta_of(second, offs, i, 1).tobytes() == starts[i].tobytes(), i      # the stopped cadence did not move the start
		assert second['flux'][i, 1] == first['flux'][i, 2]                            # the same cadence from the same point: the same bits


def test_identity_four_and_five_stars(ctx, monkeypatch):
	"""The scene of test_psf_fit_batch_equals_target_by_target: the four- and five-star classes against the oracle's model at their own
	end points."""
	from photometry_amd import simulate, psf as hpsf
	from oracle import psf as opsf
	Nt, T, H, W = 24, 3, 13, 13
	s = simulate.make_scene(Nt, T, H, W, seed=123, max_neighbours=6, neighbour_tmag_range=(9.0, 13.5))
	simulate.fill_cubes(s, nan_fraction=0.002)
	prf = opsf.synthetic_prf(seed=5)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	offs, params0, mini = scene_inputs(s)
	counts = np.minimum(np.diff(offs), pc.MAX_STARS)
	assert {4, 5} <= set(counts.tolist()), counts
	# (twelve and fifteen parameters: none of these fits finishes within the reference's 1 500 / 500 iterations, so the limits are raised)
	res = fit(ctx, monkeypatch, model, s.stamps, s.images, s.backgrounds, offs, params0, mini, 5.0, maxiter=(8000, 4000))
	print('iterations of the four- and five-star targets', res['nit'][counts >= 4, :T].tolist())
	for S in (4, 5):
		n = check_identity(res, s.images, lambda i: opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(s.stamps[i])),
			offs, mini, 5, np.flatnonzero(counts == S), f'{S} stars')
		assert n >= 1, S


def test_identity_general_path(ctx, monkeypatch):
	"""One scene of test_psf_photometry_any_grid_any_cutoff: the SPOC grid at a cut-off of 6.5, the general instantiation."""
	from photometry_amd import simulate
	Nt, T, H, W = 4, 4, 11, 11
	s = simulate.make_scene(Nt, T, H, W, seed=93, max_neighbours=2, neighbour_tmag_range=(9.0, 15.0))
	simulate.fill_cubes(s, nan_fraction=0.004)
	offs, params0, mini = scene_inputs(s)
	res = fit(ctx, monkeypatch, pe.host_model('spoc'), s.stamps, s.images, s.backgrounds, offs, params0, mini, 6.5)
	n = check_identity(res, s.images, lambda i: pe.oracle_psf('spoc', s.stamps[i]), offs, mini, 6.5, range(Nt), "('spoc', 6.5)")
	assert n >= Nt * T // 2


def test_report_worst():
	"""(last in the module) The worst measured values per path, for the record in the module docstring."""
	print('worst error measure, of the peak: cached %.2e, general %.2e, identity per mini-aperture pixel %.2e (bound %.0e)' % (
		_worst['cached'], _worst['general'], _worst['identity'], pc.BOUND))
	assert max(_worst.values()) <= pc.BOUND
