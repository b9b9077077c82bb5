# -*- coding: utf-8 -*-
"""
Halo photometry without a GPU: the restatement (tests/halo_common.py) pinned by finite differences, hand cases and scipy; the
host layer (photometry_amd/halo.py) against it; the WEIGHTMAP extension through fitsio; the default-off switch.
"""
import numpy as np
import pytest
import halo_common as hc
from photometry_amd import halo, fitsio
from photometry_amd.plugins import BasePhotometry, HaloPhotometry, load_settings
from photometry_amd.source import MemoryStampSource


def _problem(npix, ncad, seed, n_dropped=None):
	rng = np.random.default_rng(seed)
	base = rng.uniform(50, 1000, npix)
	walk = np.cumsum(rng.normal(size=ncad)) * 0.01
	P = base[None, :] * (1 + 1e-3 * np.sin(np.arange(ncad) / 7.0))[:, None] * (1 + 0.05 * walk[:, None] * rng.normal(size=npix)[None, :])
	P = (P + rng.normal(size=(ncad, npix)) * 2).astype('float32')
	fit = np.ones(ncad, dtype=bool)
	n_dropped = ncad // 20 if n_dropped is None else n_dropped
	fit[3 + rng.choice(ncad - 3, size=n_dropped, replace=False)] = False
	return P, fit


@pytest.mark.parametrize('ncad', [211, 212])
def test_gradient_matches_finite_differences(ncad):
	P, fit = _problem(30, ncad, seed=ncad, n_dropped=10)
	nf = np.count_nonzero(fit)
	assert nf % 2 == ncad % 2          # an odd and an even count of fitted cadences
	theta = np.random.default_rng(1).normal(size=30) * 0.3
	f, g = hc.objective(P, fit, theta)
	h = 1e-7
	# away from kinks: a step of h in one theta moves l_t by at most h max_p w_p |P[t,p] - l_t|, so no difference of consecutive
	# fitted l (and no order among them) can change sign within the step
	w = hc.softmax(theta)
	PF = P[fit].astype('float64')
	lF = PF @ w
	reach = h * np.max(w[None, :] * np.abs(PF - lF[:, None]))
	assert np.min(np.abs(np.diff(lF))) > 4 * reach
	assert np.min(np.abs(np.diff(np.sort(lF)))) > 4 * reach
	fd = np.array([(hc.objective(P, fit, theta + h * e, False) - hc.objective(P, fit, theta - h * e, False)) / (2 * h) for e in np.eye(30)])
	np.testing.assert_allclose(fd, g, rtol=0, atol=1e-5 * np.max(np.abs(g)))


def test_softmax_invariance():
	P, fit = _problem(20, 150, seed=3)
	theta = np.random.default_rng(2).normal(size=20)
	f0, g0 = hc.objective(P, fit, theta)
	f1, g1 = hc.objective(P, fit, theta + 3.25)
	assert abs(f1 - f0) <= 1e-13 * f0
	np.testing.assert_allclose(g1, g0, rtol=1e-10, atol=1e-14)


def test_degenerate_problems():
	P, fit = _problem(5, 10, seed=4)
	fit[:] = False
	fit[:2] = True
	assert np.isnan(hc.objective(P, fit, np.zeros(5))[0])
	assert hc.lbfgs(P, fit)['status'] == hc.DEGENERATE
	assert hc.lbfgs(-np.abs(P), np.ones(10, bool))['status'] == hc.DEGENERATE   # median <= 0


# -- host part: hand cases --------------------------------------------------------------------------------------------------
def _both_splits(sector, time, timecorr=None):
	timecorr = np.zeros(len(time)) if timecorr is None else timecorr
	a, b = halo.split_times(sector, time, timecorr), hc.split_times(sector, time, timecorr)
	assert a == b
	return a


def test_split_times_sector_table():
	t = np.linspace(1338.0, 1352.0, 500)
	assert _both_splits(1, t) == (1339., 1347.366, 1349.315)
	assert _both_splits(2, np.linspace(1360.0, 1375.0, 300)) == (1368.,)
	assert _both_splits(3, np.linspace(1390.0, 1400.0, 300)) == (1395.52,)
	assert _both_splits(8, np.linspace(1520.0, 1540.0, 300)) == (1529.50,)
	# only the split times inside the time range survive; none left -> None
	assert _both_splits(1, np.linspace(1340.0, 1348.0, 100)) == (1347.366,)
	assert _both_splits(2, np.linspace(1370.0, 1380.0, 100)) is None


def test_split_times_automatic_gap():
	t = np.concatenate([np.arange(0, 12, 0.02), np.arange(13.0, 25, 0.02)]) + 1600.0
	tc = np.full(len(t), 0.001)
	st = _both_splits(20, t + tc, tc)
	i = np.flatnonzero(np.diff(t) > 0.5)[0]
	assert st == (0.5 * (t[i] + t[i + 1]) + 0.001,)
	# two gaps in the middle: no split
	t2 = np.concatenate([np.arange(0, 9, 0.02), np.arange(10, 15, 0.02), np.arange(16, 25, 0.02)]) + 1600.0
	assert _both_splits(20, t2) is None
	# a gap outside 30 % - 70 % of the sector: no split
	t3 = np.concatenate([np.arange(0, 3, 0.02), np.arange(4, 25, 0.02)]) + 1600.0
	assert _both_splits(20, t3) is None
	# NaN times are ignored
	t4 = t.copy()
	t4[::7] = np.nan
	assert _both_splits(20, t4)[0] == pytest.approx(st[0] - 0.001, abs=0.05)


def test_segments():
	t = np.array([1, 2, np.nan, 3, 4, 5.0])
	np.testing.assert_array_equal(halo.segments(t, (3.0,)), [0, 0, -1, 1, 1, 1])
	np.testing.assert_array_equal(halo.segments(t, None), [0, 0, -1, 0, 0, 0])
	np.testing.assert_array_equal(hc.segments(t, (3.0,)), halo.segments(t, (3.0,)))


def test_pixel_mask_hand_cases():
	# one column of 25 rows: 1-based rows 1 .. 25 at column 1; target at (row 0, column 1) -> dist = row; 20 is inside
	stamp = (0, 25, 0, 1)
	ap = np.ones((25, 1), dtype='int32')
	ap[3, 0] = 2                     # bit 1 not set
	cols, rows = np.meshgrid(np.arange(1, 2, dtype='int32'), np.arange(1, 26, dtype='int32'))
	m = halo.pixel_mask(ap, cols, rows, 0.0, 1.0)
	np.testing.assert_array_equal(m, hc.pixel_mask(ap, stamp, 0.0, 1.0))
	assert m[19, 0] and not m[20, 0]     # row 20: dist exactly 20; row 21 out
	assert not m[3, 0] and m[4, 0]
	# the 1-based grid: a target at stamp pixel (2, 2) 0-based is at distance 1 from it, (3, 3) is the zero-distance pixel
	cols, rows = np.meshgrid(np.arange(1, 6, dtype='int32'), np.arange(1, 6, dtype='int32'))
	m = halo.pixel_mask(np.ones((5, 5), 'int32'), cols, rows, 2.0, 2.0, dist_max=0.0)
	assert m[1, 1] and m.sum() == 1


def test_settings_other_than_the_reference_raise():
	halo.check_settings(**halo.SETTINGS)
	for key, value in (('thresh', 0.8), ('sub', 2), ('sigclip', True), ('objective', 'tv_o2'), ('random_init', True), ('minflux', 0.0)):
		with pytest.raises(ValueError):
			halo.check_settings(**{key: value})


def test_problems_and_packing_follow_the_restatement():
	rng = np.random.default_rng(5)
	R, C, T = 6, 5, 40
	images = (rng.uniform(10, 100, (R, C, T))).astype('float32')
	images[1, 1, 7] = np.nan
	images[0, 0, :] = -500.0                       # below minflux: dropped
	quality = np.zeros(T, 'int32')
	quality[[3, 30]] = 32
	mask = np.ones((R, C), bool)
	mask[5, 4] = False
	time = np.linspace(1365, 1371, T)
	seg = halo.segments(time, halo.split_times(2, time, np.zeros(T)))
	mine = halo.build_problems(images, quality, mask, seg)
	ref = hc.problems(images, quality, mask, seg)
	assert len(mine) == len(ref) == 2
	for a, b in zip(mine, ref):
		np.testing.assert_array_equal(a.pix, b['pix'])
		np.testing.assert_array_equal(a.cad, b['cad'])
		np.testing.assert_array_equal(a.P, b['P'])
		np.testing.assert_array_equal(a.fit, b['fit'])
	assert 0 not in mine[0].pix and 7 not in mine[0].cad
	P, fit, offset, npix, ncad = halo.pack(mine)
	assert np.all(offset % 4 == 0)
	for i, p in enumerate(mine):
		pitch = (npix[i] + 3) // 4 * 4
		block = P[offset[i]:offset[i] + pitch * ncad[i]].reshape(ncad[i], pitch)
		np.testing.assert_array_equal(block[:, :npix[i]], p.P)
		assert not block[:, npix[i]:].any()


def test_flux_err_and_weightmap_identity():
	rng = np.random.default_rng(6)
	R, C, T = 5, 4, 30
	images = rng.uniform(100, 200, (R, C, T)).astype('float32')
	err = rng.uniform(1, 2, (R, C, T)).astype('float32')
	mask = np.ones((R, C), bool)
	time = np.linspace(1365, 1371, T)
	time[4] = np.nan
	seg = hc.segments(time, hc.split_times(2, time, np.zeros(T)))
	probs = hc.problems(images, np.zeros(T, 'int32'), mask, seg)
	wms = []
	for k, p in enumerate(probs):
		w = hc.softmax(rng.normal(size=p['P'].shape[1]))
		lc, med = hc.light_curve(p['P'], p['fit'], w)
		wm = halo.weightmap((R, C), p['pix'], w, med)
		np.testing.assert_array_equal(wm, hc.weightmap((R, C), p['pix'], w, med))
		# sum(wm * image) = corr_flux at every cadence of the segment
		for j, t in enumerate(p['cad']):
			assert np.sum(wm * images[:, :, t].astype('float64')) == pytest.approx(lc[j] / med, rel=1e-12)
		wms.append(wm)
	fe = halo.flux_err(wms, seg, err, 1234.5)
	for k in range(T):
		if seg[k] < 0:
			assert fe[k] == 0
		else:
			assert fe[k] == pytest.approx(1234.5 * np.sqrt(np.sum(wms[seg[k]]**2 * err[:, :, k].astype('float64')**2)), rel=1e-12)
	np.testing.assert_allclose(hc.flux_err(wms, seg, err, 20.451 - 2.5 * np.log10(1234.5)), fe, rtol=1e-9)


# -- the WEIGHTMAP extension -------------------------------------------------------------------------------------------------
def _region_source(R=30, C=28, T=12, row0=40, col0=60):
	rng = np.random.default_rng(8)
	frames = {k: rng.uniform(1, 2, (R, C, T)).astype('float32') for k in ('images', 'images_err', 'backgrounds')}
	cat = {'starid': np.array([1, 2]), 'tmag': np.array([5.0, 12.0], dtype='float32'),
		'row': np.array([55.2, 47.0], dtype='float32'), 'column': np.array([73.7, 66.0], dtype='float32')}
	return MemoryStampSource(frames, row0, col0, 1365.0 + np.arange(T) * 0.02, np.zeros(T), np.arange(T), np.zeros(T, dtype='int32'), cat,
		sector=2)


def test_weightmap_extension_round_trip(tmp_path):
	src = _region_source()
	with BasePhotometry(1, src, str(tmp_path), datasource='ffi') as pho:
		pho.resize_stamp(width=22, height=22)
		H, W = pho.stamp[1] - pho.stamp[0], pho.stamp[3] - pho.stamp[2]
		pho._sumimage = np.ones((H, W))
		pho.lightcurve['flux'] = np.ones(pho.Ntimes)
		rng = np.random.default_rng(9)
		wms = [rng.uniform(0, 1e-3, (H, W)), rng.uniform(0, 1e-3, (H, W))]
		pho.halo_weightmap = {'weightmap': wms, 'initial_cadence': [0, 6], 'final_cadence': [5, 11], 'sat_pixels': [0, 0]}
		path = pho.save_lightcurve()
	hdus = fitsio.read(path)
	assert len(hdus) == 5
	assert hdus[0][0]['NEXTEND'] == 4
	hdr, data = hdus[4]
	assert hdr['EXTNAME'] == 'WEIGHTMAP' and hdr['__checksum_ok__'] and hdr['__datasum_ok__']
	assert hdr['TFORM4'] == f'{H * W:d}E' and hdr['TDIM4'] == f'({W:d},{H:d})'
	assert [hdr[f'TTYPE{i}'] for i in range(1, 5)] == ['CADENCENO1', 'CADENCENO2', 'SAT_PIXELS', 'WEIGHTMAP']
	np.testing.assert_array_equal(data['CADENCENO1'], [0, 6])
	np.testing.assert_array_equal(data['CADENCENO2'], [5, 11])
	assert data['WEIGHTMAP'].shape == (2, H, W)
	np.testing.assert_array_equal(data['WEIGHTMAP'], np.asarray(wms, dtype='float32'))
	# the raw cards as the reference writes them
	raw = open(path, 'rb').read() if not path.endswith('.gz') else __import__('gzip').open(path).read()
	assert b"TDIM4   = '(%d,%d)" % (W, H) in raw and b"TFORM4  = '%dE" % (H * W) in raw


def test_without_weightmap_nothing_changes(tmp_path):
	src = _region_source()
	with BasePhotometry(1, src, str(tmp_path), datasource='ffi') as pho:
		pho._sumimage = np.ones((pho.stamp[1] - pho.stamp[0], pho.stamp[3] - pho.stamp[2]))
		pho.lightcurve['flux'] = np.ones(pho.Ntimes)
		hdus = fitsio.read(pho.save_lightcurve())
	assert len(hdus) == 4 and hdus[0][0]['NEXTEND'] == 3


# -- off by default ----------------------------------------------------------------------------------------------------------
def test_halo_is_off_by_default(monkeypatch, tmp_path):
	monkeypatch.delenv('TESSPHOT_SETTINGS', raising=False)
	assert load_settings().get('halo', 'enabled') == 'false'
	assert not HaloPhotometry.is_available() and not halo.enabled()
	with HaloPhotometry(1, _region_source(), str(tmp_path)) as pho:
		with pytest.raises(NotImplementedError, match=r'\[halo\] enabled = true'):
			pho.do_photometry()
	ini = tmp_path / 'settings.ini'
	ini.write_text('[halo]\nenabled = true\n')
	monkeypatch.setenv('TESSPHOT_SETTINGS', str(ini))
	assert HaloPhotometry.is_available() and halo.enabled()
	assert load_settings().getfloat('haloswitch', 'tmag_limit') == 6.0


# -- the optimiser against scipy ---------------------------------------------------------------------------------------------
def test_restated_optimiser_against_scipy():
	opt = pytest.importorskip('scipy.optimize')
	rng = np.random.default_rng(10)
	ratios = []
	for k in range(20):
		P, fit = _problem(int(rng.integers(2, 60)), int(rng.integers(20, 300)), seed=100 + k)
		mine = hc.lbfgs(P, fit)
		ref = opt.minimize(lambda th: hc.objective(P, fit, th), np.zeros(P.shape[1]), jac=True, method='L-BFGS-B', options={'maxiter': 101})
		assert mine['status'] in (hc.CONVERGED, hc.CAP_REACHED, hc.LINESEARCH_FAILED)
		assert np.all(mine['w'] >= 0) and abs(np.sum(mine['w']) - 1) < 1e-12
		ratios.append(mine['f'] / ref.fun)
	assert max(ratios) <= 1.05, ratios
