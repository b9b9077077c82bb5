# -*- coding: utf-8 -*-
"""
The 'wcs' movement kernel on the device (csrc/wcs.hip, photometry_amd/wcs.py, MovementKernel('wcs')) against astropy's and the
reference's own outputs (golden_wcs.npz) and the spherical-trigonometry restatement tests/wcs_common.py; the known answers of the
reference's tests/test_imagemotion.py; reproducibility; linpsf_frames(movement=wcs) against the LinPSF plugin; and per-star
positions of a field that rotates from frame to frame.
"""
import os
import numpy as np
import pytest
import wcs_common as wc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'golden_wcs.npz')


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.fixture(scope='module')
def g():
	return dict(np.load(GOLDEN))


def _card(key, value):
	return f"{key:<8}= {value:>20}".ljust(80)


def _header(crpix=(1045.0, 1001.0), crval=(84.1, -62.3), rot=0.0, sip=True):
	s = 21.0 / 3600
	c, n = np.cos(np.deg2rad(rot)), np.sin(np.deg2rad(rot))
	cd = s * np.array([[-c, n], [n, c]])
	cards = [('CTYPE1', "'RA---TAN" + ("-SIP'" if sip else "'")), ('CTYPE2', "'DEC--TAN" + ("-SIP'" if sip else "'")),
		('CRPIX1', repr(float(crpix[0]))), ('CRPIX2', repr(float(crpix[1]))), ('CRVAL1', repr(float(crval[0]))), ('CRVAL2', repr(float(crval[1]))),
		('CD1_1', repr(float(cd[0, 0]))), ('CD1_2', repr(float(cd[0, 1]))), ('CD2_1', repr(float(cd[1, 0]))), ('CD2_2', repr(float(cd[1, 1])))]
	if sip:
		cards += [('A_ORDER', '3'), ('B_ORDER', '3'), ('A_2_0', '2.1E-6'), ('A_1_1', '-1.3E-6'), ('A_0_2', '0.7E-6'), ('A_3_0', '1.1E-9'),
			('B_2_0', '-0.4E-6'), ('B_1_1', '1.9E-6'), ('B_0_2', '-1.2E-6'), ('B_0_3', '0.8E-9')]
	return ''.join(_card(k, v) for k, v in cards)


def test_transforms_against_astropy(ctx, g):
	from photometry_amd.wcs import TanSipWCS, DIVERGENT, SLOW
	for i, name in enumerate(g['hdr_names']):
		w = TanSipWCS.from_header(str(g['hdr_strings'][i]), ctx=ctx)
		pts = g[f'hdr_{i}_pix']
		a = w.all_pix2world(pts, 0)
		assert wc.ra_diff(a[:, 0], g[f'hdr_{i}_all_pix2world'][:, 0]).max() < 1e-10, name
		assert np.abs(a[:, 1] - g[f'hdr_{i}_all_pix2world'][:, 1]).max() < 1e-10, name
		a1 = w.all_pix2world(pts, 1)
		assert wc.ra_diff(a1[:, 0], g[f'hdr_{i}_all_pix2world_o1'][:, 0]).max() < 1e-10, name
		b = w.wcs_pix2world(pts[:, 0], pts[:, 1], 0)
		assert wc.ra_diff(b[0], g[f'hdr_{i}_wcs_pix2world'][:, 0]).max() < 1e-10, name
		assert np.abs(w.pix2foc(pts, 0) - g[f'hdr_{i}_pix2foc']).max() < 1e-10, name
		fp = w.calc_footprint(axes=(2136, 2078))
		assert wc.ra_diff(fp[:, 0], g[f'hdr_{i}_footprint'][:, 0]).max() < 1e-10, name
		assert np.abs(fp[:, 1] - g[f'hdr_{i}_footprint'][:, 1]).max() < 1e-10, name
		fp22 = w.calc_footprint(axes=(2, 2))
		assert wc.ra_diff(fp22[:, 0], g[f'hdr_{i}_footprint22'][:, 0]).max() < 1e-10, name
		assert np.abs(fp22[:, 1] - g[f'hdr_{i}_footprint22'][:, 1]).max() < 1e-10, name
		for bt in (0, 1):
			world = g[f'hdr_{i}_world{bt}']
			np.testing.assert_allclose(w.wcs_world2pix(world, 0), g[f'hdr_{i}_wcs_world2pix{bt}'], rtol=0, atol=1e-8, err_msg=name)
			pix = w.all_world2pix(world, 0, quiet=True)
			assert w.last_iterations == int(g[f'hdr_{i}_iters{bt}']), (name, bt, w.last_iterations)
			np.testing.assert_array_equal((w.last_status & DIVERGENT) != 0, g[f'hdr_{i}_divergent{bt}'], err_msg=name)
			np.testing.assert_array_equal((w.last_status & SLOW) != 0, g[f'hdr_{i}_slow{bt}'], err_msg=name)
			ok = ~g[f'hdr_{i}_divergent{bt}']
			np.testing.assert_allclose(pix[ok], g[f'hdr_{i}_all_world2pix{bt}'][ok], rtol=0, atol=1e-8, err_msg=name)


def test_transforms_against_restatement(ctx, g):
	from photometry_amd.wcs import TanSipWCS
	rng = np.random.default_rng(4)
	for i, name in enumerate(g['hdr_names']):
		s = str(g['hdr_strings'][i])
		w, r = TanSipWCS.from_header(s, ctx=ctx), wc.RefWCS(s)
		pts = np.column_stack((rng.uniform(-100, 2200, 500), rng.uniform(-100, 2150, 500)))
		a, ra = w.all_pix2world(pts, 0), r.all_pix2world(pts, 0)
		assert wc.ra_diff(a[:, 0], ra[:, 0]).max() < 1e-10 and np.abs(a[:, 1] - ra[:, 1]).max() < 1e-10, name
		world = ra + rng.normal(0, 0.02, ra.shape)
		for batch in (world, world[:7], world[:1]):
			pix = w.all_world2pix(batch, 0, quiet=True)
			rp, k, div, slow = r.all_world2pix(batch, 0)
			assert w.last_iterations == k, (name, len(batch))
			np.testing.assert_array_equal((w.last_status & 1) != 0, div)
			np.testing.assert_allclose(pix[~div], rp[~div], rtol=0, atol=1e-8, err_msg=name)


def test_all_world2pix_raises_without_quiet(ctx, g):
	from photometry_amd.wcs import TanSipWCS, NoConvergence
	i = list(g['hdr_names']).index('divergent')
	w = TanSipWCS.from_header(str(g['hdr_strings'][i]), ctx=ctx)
	with pytest.raises(NoConvergence):
		w.all_world2pix(w.calc_footprint(axes=(2, 2))[:1], 0, maxiter=50)


def test_known_answers(ctx):
	"""tests/test_imagemotion.py:114-197 of the reference: the same WCS moves nothing; CRPIX + 1 without SIP moves by one pixel."""
	from photometry_amd.motion import MovementKernel
	xy = np.array([[100.5, 200.25], [1500.0, 30.0], [1000.0, 1000.0], [2100.0, 2050.0]])
	mk = MovementKernel('wcs', wcs_ref=_header(), ctx=ctx)
	assert np.abs(mk.apply_kernel(xy, _header())).max() <= 1e-5
	mk0 = MovementKernel('wcs', wcs_ref=_header(sip=False), ctx=ctx)
	j = mk0.apply_kernel(xy, _header(crpix=(1046.0, 1002.0), sip=False))
	np.testing.assert_allclose(j, 1.0, rtol=0, atol=1e-12)


def _drifting(T, rot_arcsec=30.0, seed=2):
	rng = np.random.default_rng(seed)
	return [_header(crval=(84.1 + rng.normal(0, 1.0 / 3600), -62.3 + rng.normal(0, 1.0 / 3600)), rot=rot_arcsec / 3600 * np.sin(k / 3.0))
		for k in range(T)]


def test_bit_identical_runs_and_chunkings(ctx):
	from photometry_amd import wcs as W
	ref = W.TanSipWCS.from_header(_header())
	frames = [W.TanSipWCS.from_header(h) for h in _drifting(37)]
	rng = np.random.default_rng(0)
	xy = np.column_stack((rng.uniform(0, 2100, 300), rng.uniform(0, 2050, 300)))
	offsets = np.array([0, 30, 31, 200, 300])
	d_cos = W.world_directions(ctx, ref, xy)
	allp = ctx.array(W.pack(frames))
	a = W.world2pix_frames(ctx, allp, 37, d_cos, 300, offsets)
	b = W.world2pix_frames(ctx, allp, 37, d_cos, 300, offsets)
	p1, p2 = ctx.array(W.pack(frames[:20])), ctx.array(W.pack(frames[20:]))
	c1 = W.world2pix_frames(ctx, p1, 20, d_cos, 300, offsets)
	c2 = W.world2pix_frames(ctx, p2, 17, d_cos, 300, offsets)
	for x, y in zip(a, b):
		assert np.array_equal(x, y)
	for k in range(3):
		assert np.array_equal(a[k], np.concatenate((c1[k], c2[k])))
	assert np.all(a[1] == 0) and np.all(a[2] >= 2)


def test_movement_kernel_against_reference(ctx, g):
	from photometry_amd.motion import MovementKernel
	mk = MovementKernel('wcs', wcs_ref=str(g['series_ref']), ctx=ctx)
	mk.load_series(g['series_times'], [str(h) for h in g['series_headers']])
	np.testing.assert_array_equal(mk.series_times, g['series_times'][g['series_kept']])
	xy = g['series_xy']
	for t, ref in zip(g['series_query'], g['series_interpolate']):
		np.testing.assert_allclose(mk.interpolate(t, xy), ref, rtol=0, atol=1e-8)
	for t in g['series_bad_query']:
		with pytest.raises(ValueError, match='outside'):
			mk.interpolate(t, xy)
	at = g['series_jitter_at']
	np.testing.assert_allclose(mk.jitter(g['series_jitter_time'], at[0], at[1]), g['series_jitter'], rtol=0, atol=1e-8)


def test_movement_from_stack_header(ctx, tmp_path, g):
	from photometry_amd import frameio, motion
	T = len(g['series_times'])
	path = str(tmp_path / 'w.tpstack')
	frameio.write_stack(path, {'images': np.zeros((T, 4, 5), dtype='float32')}, time=g['series_times'],
		movement_kernel=np.zeros((T, 2)), wcs_headers=[str(h) for h in g['series_headers']], wcs_ref=str(g['series_ref']))
	hdr = frameio.read_header(path)
	mk = motion.movement_from_header(hdr)
	assert mk.warpmode == 'wcs'
	mk.ctx = ctx
	at = g['series_jitter_at']
	np.testing.assert_allclose(mk.jitter(g['series_jitter_time'], at[0], at[1]), g['series_jitter'], rtol=0, atol=1e-8)


def _rotating_scene(T=12):
	"""WCS headers of a field whose CD matrix turns by 40 arcsec per frame about CRPIX (1045, 1001), inside the sampled region:
	the shifts grow with the distance from CRPIX, so they differ from star to star."""
	hdrs = [_header(crpix=(1045.0, 1001.0), rot=40.0 / 3600 * k) for k in range(T)]
	return hdrs


def test_positions_of_a_rotating_field_equal_restatement(ctx):
	from photometry_amd import wcs as W
	T = 12
	hdrs = _rotating_scene(T)
	ref = W.TanSipWCS.from_header(hdrs[0])
	frames = [W.TanSipWCS.from_header(h) for h in hdrs]
	rng = np.random.default_rng(9)
	n = 200
	xy32 = np.column_stack((rng.uniform(0, 2100, n), rng.uniform(0, 2050, n))).astype('float32')
	base = (xy32 - np.float32(100.0)).astype('float32')
	offsets = np.array([0, 1, 40, 41, 120, 200])
	out_index = np.where(rng.random(n) < 0.7, 0, -1)
	out_index[out_index == 0] = np.arange((out_index == 0).sum())
	n_out = int((out_index >= 0).sum())
	times = np.arange(T, dtype='float64')
	t = np.concatenate((times, times[:-1] + 0.37))
	k1 = np.concatenate((np.arange(T), np.arange(T - 1))).astype('int32')
	k2 = np.concatenate((np.full(T, -1), np.arange(1, T))).astype('int32')
	dt = np.where(k2 >= 0, times[np.maximum(k2, 0)] - times[k1], 0.0)
	dx = t - times[k1]
	pc, pr, st = W.star_positions(ctx, ctx.array(W.pack(frames)), T, ref, offsets, xy32, base[:, 0], base[:, 1], out_index, n_out, k1, k2, dt, dx)
	pc, pr = pc.to_host()[:n_out], pr.to_host()[:n_out]
	assert np.all(st == 0)
	# the restatement: one batch per stamp catalogue, jitter = all_world2pix(ref.all_pix2world(xy)) - xy
	r_ref = wc.RefWCS(hdrs[0])
	exp_c = np.empty((n_out, len(t)))
	exp_r = np.empty((n_out, len(t)))
	xy = xy32.astype('float64')
	for b in range(len(offsets) - 1):
		lo, hi = offsets[b], offsets[b + 1]
		world = r_ref.all_pix2world(xy[lo:hi], 0)
		jf = np.array([wc.RefWCS(h).all_world2pix(world, 0, maxiter=50)[0] - xy[lo:hi] for h in hdrs])     # (T, m, 2)
		for k in range(len(t)):
			j = jf[k1[k]] if k2[k] < 0 else (jf[k2[k]] - jf[k1[k]]) / dt[k] * dx[k] + jf[k1[k]]
			for m in range(lo, hi):
				if out_index[m] >= 0:
					exp_c[out_index[m], k] = base[m, 0] + j[m - lo, 0]
					exp_r[out_index[m], k] = base[m, 1] + j[m - lo, 1]
	# float32 sums: the device forms float64(float32(base + jitter)); the restatement's jitter agrees to 1e-8 px, so the two
	# round to the same float32 but where the sum lies within 1e-8 of a rounding boundary (then one float32 step apart)
	for got, exp in ((pc, exp_c), (pr, exp_r)):
		e32 = exp.astype('float32')
		step = np.spacing(np.abs(e32)).astype('float64')
		assert np.all(np.abs(got - e32) <= step)
		assert np.mean(got == e32) > 0.99
	# the field rotates: stars at different places move differently
	spread = np.ptp(pc[:, T - 1] - pc[:, 0])
	assert spread > 0.1


def test_linpsf_frames_wcs_equals_plugin(ctx, tmp_path):
	from photometry_amd import pipeline, STATUS
	from photometry_amd import psf as hpsf, simulate
	from photometry_amd.motion import MovementKernel
	from photometry_amd.plugins import LinPSFPhotometry
	from photometry_amd.source import MemoryStampSource
	from test_gpu_psf_frames import _region
	T = 10
	frames, row0, col0, time, quality, cat, targets, _ = _region(T=T)
	prf = simulate.synthetic_prf(seed=3)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	stack = pipeline.FrameStack(ctx, {k: np.moveaxis(v, 2, 0) for k, v in frames.items()}, row0, col0)
	hdrs = [_header(crpix=(300.0, 150.0), rot=60.0 / 3600 * np.sin(k)) for k in range(T)]
	hdrs[4] = ''
	timecorr = np.full(T, 1e-4)
	mk = MovementKernel('wcs', wcs_ref=hdrs[0], ctx=ctx)
	mk.load_series(time - timecorr, hdrs)
	assert len(mk.series_times) == T - 1
	batch = pipeline.linpsf_frames(ctx, stack, targets, cat, time, quality, model, movement=mk, timecorr=timecorr)
	src = MemoryStampSource(frames, row0, col0, time, timecorr, np.arange(T), quality, cat, targets=targets, prf=model, movement=mk)
	for i in range(len(targets['starid'])):
		b = batch[i]
		with LinPSFPhotometry(int(targets['starid'][i]), src, str(tmp_path), ctx=ctx) as pho:
			status = pho.do_photometry()
			assert tuple(pho.stamp) == b['stamp']
			assert status.value == b['status']
			np.testing.assert_array_equal(pho.lightcurve['flux'], b['flux'])
			np.testing.assert_array_equal(pho.lightcurve['flux_err'], b['flux_err'])
			pc = pho.lightcurve['pos_corr']
			np.testing.assert_array_equal(pc, mk.jitter(time - timecorr, pho.target_pos_column, pho.target_pos_row))
			assert status != STATUS.ERROR


def test_source_projects_ra_dec(ctx):
	from photometry_amd.source import MemoryStampSource
	from photometry_amd.wcs import TanSipWCS
	h = _header()
	w = TanSipWCS.from_header(h, ctx=ctx)
	px = np.array([[100.25, 200.5], [110.0, 190.0], [1500.5, 30.25]])
	world = w.all_pix2world(px, 0)
	T = 2
	frames = {'images': np.zeros((4, 4, T), dtype='float32')}
	cat = {'starid': np.arange(3), 'tmag': np.ones(3, dtype='float32'), 'ra': world[:, 0], 'dec': world[:, 1]}
	src = MemoryStampSource(frames, 0, 0, np.arange(T), np.zeros(T), np.arange(T), np.zeros(T), cat, wcs=h,
		targets={'starid': np.array([0]), 'tmag': np.array([1.0]), 'ra': world[:1, 0], 'dec': world[:1, 1]})
	np.testing.assert_allclose(src.catalog['column'], px[:, 0].astype('float32'), rtol=0, atol=1e-4)
	assert src.catalog['row'].dtype == np.float32
	tgt = src.target(0)
	assert abs(tgt['column'] - 100.25) < 1e-8 and abs(tgt['row'] - 200.5) < 1e-8


def test_empty_batches(ctx):
	"""Empty batches (equal offsets, and n == 0 with no point array at all) read and write nothing and count no iteration."""
	from photometry_amd import wcs as W
	ref = W.TanSipWCS.from_header(_header())
	frames = [W.TanSipWCS.from_header(h) for h in _drifting(3)]
	d_params = ctx.array(W.pack(frames))
	xy = np.array([[100.5, 200.25], [1500.0, 30.0], [1000.0, 1000.0]])
	d_cos = W.world_directions(ctx, ref, xy)
	alone = W.world2pix_frames(ctx, d_params, 3, d_cos, 3, [0, 3])
	pix, st, it = W.world2pix_frames(ctx, d_params, 3, d_cos, 3, [0, 0, 3, 3])
	assert np.array_equal(pix, alone[0]) and np.array_equal(st, alone[1])
	assert np.array_equal(it[:, 1], alone[2][:, 0]) and np.all(it[:, [0, 2]] == 0)
	# n == 0: d_cos may be NULL (tp_wcs_world2pix); two empty batches
	offsets = np.zeros(3, dtype='int64')
	d_pix, d_st, d_it = ctx.empty((3, 1, 2), 'float64'), ctx.empty((3, 1), 'int32'), ctx.array(np.full((3, 2), -7, dtype='int32'))
	ctx._check(ctx.lib.tp_wcs_world2pix(ctx.handle, d_params.ptr, 3, 0, 2, offsets.ctypes.data, None, 0, 1, 1e-4, 20, d_pix.ptr, d_st.ptr, d_it.ptr))
	assert np.all(d_it.to_host() == 0)
	# LinPSF positions: an empty stamp catalogue between two others, and one at the end (lo == n)
	xy32 = xy.astype('float32')
	k1 = np.arange(3, dtype='int32')
	k2 = np.full(3, -1, dtype='int32')
	z = np.zeros(3)
	one = W.star_positions(ctx, d_params, 3, ref, [0, 1, 3], xy32, xy32[:, 0], xy32[:, 1], np.arange(3), 3, k1, k2, z, z)
	gap = W.star_positions(ctx, d_params, 3, ref, [0, 1, 1, 3, 3], xy32, xy32[:, 0], xy32[:, 1], np.arange(3), 3, k1, k2, z, z)
	for a, b in zip(one[:2], gap[:2]):
		assert np.array_equal(a.to_host(), b.to_host())
	assert np.array_equal(one[2], gap[2])


def test_source_projection_raises_like_the_reference(ctx, g):
	"""BasePhotometry.py:1159 / :461 call all_world2pix without quiet: a catalogue point that does not converge raises."""
	from photometry_amd.source import MemoryStampSource
	from photometry_amd.wcs import TanSipWCS, NoConvergence
	i = list(g['hdr_names']).index('divergent')
	h = str(g['hdr_strings'][i])
	corner = TanSipWCS.from_header(h, ctx=ctx).calc_footprint(axes=(2, 2))[:1]
	T = 2
	cat = {'starid': np.arange(1), 'tmag': np.ones(1, dtype='float32'), 'ra': corner[:, 0], 'dec': corner[:, 1]}
	with pytest.raises(NoConvergence):
		MemoryStampSource({'images': np.zeros((4, 4, T), dtype='float32')}, 0, 0, np.arange(T), np.zeros(T), np.arange(T), np.zeros(T), cat, wcs=h)
