# -*- coding: utf-8 -*-
"""
Halo photometry on the device (csrc/halo.hip, photometry_amd/halo.py) against the CPU restatement (tests/halo_common.py):
the objective and its gradient, the L-BFGS optimiser, bit-reproducibility, a known-answer star and the automatic switch of
``tessphot(None, ...)`` for a bright target whose aperture run gave up.
"""
import numpy as np
import pytest
from scipy.special import erf
import halo_common as hc

pytestmark = pytest.mark.gpu

NPIX = (1, 63, 64, 484, 1257)
NCAD = (3, 1299, 1300, 19000)


def _problem(npix, ncad, seed):
	rng = np.random.default_rng(seed)
	base = rng.uniform(50, 1000, npix)
	walk = np.cumsum(rng.normal(size=ncad)) * 0.01
	P = base[None, :] * (1 + 1e-3 * np.sin(np.arange(ncad) / 7.0))[:, None] * (1 + 0.05 * walk[:, None] * rng.normal(size=npix)[None, :])
	P = (P + rng.normal(size=(ncad, npix)) * 2).astype('float32')
	fit = rng.random(ncad) >= 0.05
	if ncad <= 3:
		fit[:] = True
	return P, fit


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _settings_on(monkeypatch, tmp_path):
	ini = tmp_path / 'settings.ini'
	ini.write_text('[halo]\nenabled = true\n')
	monkeypatch.setenv('TESSPHOT_SETTINGS', str(ini))


def test_objective_against_the_restatement(ctx):
	from photometry_amd import halo
	shapes = [(p, c) for p in NPIX for c in NCAD]
	rng = np.random.default_rng(1)
	probs, thetas = [], []
	for i in range(50):
		npix, ncad = shapes[i % len(shapes)]
		probs.append(_problem(npix, ncad, seed=i))
		thetas.append(rng.normal(size=npix) * 0.5)
	f, grads = halo.objective(ctx, probs, thetas)
	# f is a sum of differences of l: l_t (a float64 sum of npix products) carries a rounding of order eps |l_t| in either
	# implementation, so besides 1e-12 relative the bound allows 1e-14 of sum_j (|l_j| + |l_j+1|) / m -- what dominates when few
	# cadences differ little (3 cadences: measured 1.6e-12 relative, DESIGN.md "Halo")
	bad, worst_f, worst_g = [], 0.0, 0.0
	for i, ((P, fit), th) in enumerate(zip(probs, thetas)):
		fr, gr = hc.objective(P, fit, th)
		assert np.isfinite(fr), i
		lF = P[fit].astype('float64') @ hc.softmax(th)
		scale = np.sum(np.abs(lF[1:]) + np.abs(lF[:-1])) / np.median(lF)
		ef = abs(f[i] - fr)
		dg, gmax = np.max(np.abs(grads[i] - gr)), np.max(np.abs(gr))   # one pixel: the gradient is exactly zero in both
		worst_f = max(worst_f, ef / abs(fr))
		worst_g = max(worst_g, dg / gmax if gmax else dg)
		if not (ef <= 1e-12 * abs(fr) + 1e-14 * scale and dg <= 1e-10 * gmax):
			bad.append((i, P.shape, ef / abs(fr), ef / scale, dg, gmax))
	print(f"objective: worst relative f {worst_f:.2e}, worst gradient (relative to |grad|_inf) {worst_g:.2e}")
	assert not bad, bad


def test_objective_degenerate_problem_is_nan(ctx):
	from photometry_amd import halo
	P, fit = _problem(8, 10, seed=3)
	fit[:] = False
	fit[:2] = True
	f, g = halo.objective(ctx, [(P, fit), (-np.abs(P), np.ones(10, bool))], [np.zeros(8), np.zeros(8)])
	assert np.all(np.isnan(f)) and np.all(np.isnan(g[0])) and np.all(np.isnan(g[1]))


def _optimiser_shapes():
	shapes = [(1257, 19000), (64, 19000)]
	shapes += [(p, c) for p in (1, 63, 64, 484, 1257) for c in (3, 1299, 1300)]
	while len(shapes) < 64:
		shapes.append((484, 1300 - (len(shapes) % 2)))
	return shapes


@pytest.fixture(scope='module')
def batch(ctx):
	from photometry_amd import halo
	probs = [_problem(npix, ncad, seed=1000 + i) for i, (npix, ncad) in enumerate(_optimiser_shapes())]
	return probs, halo.tvmin(ctx, probs)


def test_optimiser_against_the_restatement(batch):
	probs, dev = batch
	n = len(probs)
	same_iters = close_w = 0
	worst_f = 0.0
	for i, (P, fit) in enumerate(probs):
		ref = hc.lbfgs(P, fit)
		assert dev['status'][i] == ref['status'], (i, P.shape, dev['status'][i], ref['status'], dev['iterations'][i], ref['iterations'])
		if ref['status'] == hc.DEGENERATE:
			continue
		assert dev['f'][i] <= ref['f'] * (1 + 1e-6), (i, P.shape, dev['f'][i], ref['f'])
		worst_f = max(worst_f, dev['f'][i] / ref['f'] - 1)
		same_iters += int(dev['iterations'][i] == ref['iterations'])
		close_w += int(np.max(np.abs(dev['w'][i] - ref['w'])) <= 1e-6)
		assert np.all(dev['w'][i] >= 0) and abs(np.sum(dev['w'][i]) - 1) < 1e-12
		lc, _ = hc.light_curve(P, fit, dev['w'][i])
		np.testing.assert_allclose(dev['l'][i], lc, rtol=1e-12)
	print(f"optimiser: {same_iters}/{n} equal iteration counts, {close_w}/{n} weights within 1e-6, worst f excess {worst_f:.2e}")
	assert same_iters >= 0.9 * n and close_w >= 0.9 * n, (same_iters, close_w)


def test_bit_reproducible_and_batch_independent(ctx, batch):
	from photometry_amd import halo
	probs, dev = batch
	again = halo.tvmin(ctx, probs)
	for key in ('f', 'iterations', 'status'):
		assert np.array_equal(again[key], dev[key], equal_nan=True), key
	for i in range(len(probs)):
		assert np.array_equal(again['w'][i], dev['w'][i]) and np.array_equal(again['l'][i], dev['l'][i]), i
	for i in (0, 20, len(probs) - 1):
		alone = halo.tvmin(ctx, [probs[i]])
		assert np.array_equal(alone['w'][0], dev['w'][i]) and np.array_equal(alone['l'][0], dev['l'][i]), i
		assert alone['f'][0] == dev['f'][i] and alone['iterations'][0] == dev['iterations'][i] and alone['status'][0] == dev['status'][i]


def test_known_answer_bright_star(monkeypatch, tmp_path):
	from photometry_amd import tessphot, STATUS, fitsio
	from photometry_amd.plugins import HaloPhotometry, mag2flux
	from photometry_amd.source import MemoryStampSource
	_settings_on(monkeypatch, tmp_path)
	sc = hc.bright_star_scene()
	src = MemoryStampSource(sc['frames'], sc['row0'], sc['col0'], sc['time'], sc['timecorr'], sc['cadenceno'], sc['quality'], sc['catalog'],
		sector=2, jitter=sc['jitter'], targets=sc['targets'])
	pho = tessphot('halo', sc['starid'], src, str(tmp_path / 'out'))
	assert isinstance(pho, HaloPhotometry) and pho.status == STATUS.OK, pho._details.get('errors')
	res = pho.halo_result
	assert res['split_times'] == (1368.0,) and len(res['w']) == 2 and len(pho.halo_weightmap['weightmap']) == 2
	for w in res['w']:
		assert np.all(w >= 0) and abs(np.sum(w) - 1) < 1e-12
	corr = pho.lightcurve['flux'] / mag2flux(5.0)
	seg = res['segments']
	amp, rms = hc.sinusoid_fit(sc['time'], corr, seg, sc['period'])
	# the plain sum over the same pixel mask, normalised per segment the same way
	st = pho.stamp
	cube = sc['frames']['images'][st[0] - sc['row0']:st[1] - sc['row0'], st[2] - sc['col0']:st[3] - sc['col0']]
	s = cube[pho.final_phot_mask].astype('float64').sum(axis=0)
	plain = np.full(len(s), np.nan)
	good = (sc['quality'] & hc.DEFAULT_BITMASK) == 0
	for k in range(seg.max() + 1):
		plain[seg == k] = s[seg == k] / np.median(s[(seg == k) & good])
	amp0, rms0 = hc.sinusoid_fit(sc['time'], plain, seg, sc['period'])
	print(f"known answer: amplitude {amp:.4e} (injected 1e-3), residual rms {rms:.3e} vs plain sum {rms0:.3e}")
	assert abs(amp - 1e-3) <= 0.1e-3
	assert rms <= 0.5 * rms0
	np.testing.assert_allclose(pho.lightcurve['pos_centroid'][:, 0], sc['targets']['column'][0] + sc['jitter'][:, 0])
	hdus = fitsio.read(pho.save_lightcurve())
	assert hdus[0][0]['NEXTEND'] == 4 and hdus[4][0]['EXTNAME'] == 'WEIGHTMAP' and hdus[0][0]['HALO_OBJ'] == 'tv'


def _region(seed=3, R=110, C=96, T=24):
	"""A CCD region with faint stars and a Tmag 5.5 star whose bleed trail runs into the lower frame limit: its aperture run ends
	in the haloswitch quick break."""
	rng = np.random.default_rng(seed)
	row0, col0 = 200, 300
	stars = [
		(row0 + 30.3, col0 + 25.6, 11.0, 0), (row0 + 31.9, col0 + 60.2, 9.5, 0), (row0 + 70.4, col0 + 20.7, 12.5, 0),
		(row0 + 12.1, col0 + 80.3, 5.5, 40),     # bright (Tmag < 6), trail into the lower limit
	]
	rr, cc = np.arange(R) + row0, np.arange(C) + col0
	img = np.zeros((R, C))
	for (r, c, tmag, trail) in stars:
		flux = 10**(-0.4 * (tmag - 20.451))
		sig = 0.6 if trail else 0.9
		pr = 0.5 * (erf((rr + 0.5 - r) / (np.sqrt(2) * sig)) - erf((rr - 0.5 - r) / (np.sqrt(2) * sig)))
		pc = 0.5 * (erf((cc + 0.5 - c) / (np.sqrt(2) * sig)) - erf((cc - 0.5 - c) / (np.sqrt(2) * sig)))
		img += flux * np.outer(pr, pc)
		if trail:
			ri, ci = int(round(r)) - row0, int(round(c)) - col0
			lo, hi = max(ri - trail, 0), min(ri + trail + 1, R)
			img[lo:hi, ci:ci + 2] += 0.02 * flux
	bkg = 100.0
	cube = img[:, :, None] * (1 + 1e-3 * rng.normal(size=T))[None, None, :]
	noise = np.sqrt(np.abs(cube) + bkg + 100.0)
	images = (cube + 30.0 + rng.normal(size=cube.shape) * noise).astype('float32')
	images[rng.random(images.shape) < 5e-4] = np.nan
	frames = {'images': images, 'images_err': noise.astype('float32'), 'backgrounds': np.full(images.shape, bkg, dtype='float32')}
	time = 1500.0 + np.arange(T) * 1800.0 / 86400.0
	quality = np.zeros(T, dtype='int32')
	quality[5] = 32
	cat = {'starid': np.arange(len(stars), dtype='int64') + 101, 'tmag': np.array([s[2] for s in stars], dtype='float32'),
		'row': np.array([s[0] for s in stars], dtype='float32'), 'column': np.array([s[1] for s in stars], dtype='float32')}
	targets = {'starid': cat['starid'].copy(), 'tmag': np.array([s[2] for s in stars]), 'row': np.array([s[0] for s in stars]),
		'column': np.array([s[1] for s in stars])}
	return frames, row0, col0, time, quality, cat, targets


def test_auto_switch_to_halo(monkeypatch, tmp_path):
	from photometry_amd import tessphot, STATUS, fitsio
	from photometry_amd.plugins import AperturePhotometry, HaloPhotometry
	from photometry_amd.source import MemoryStampSource
	frames, row0, col0, time, quality, cat, targets = _region()
	T = len(time)

	def source():
		return MemoryStampSource(frames, row0, col0, time, np.zeros(T), np.arange(T), quality, cat, targets=targets)
	starid = 104
	monkeypatch.delenv('TESSPHOT_SETTINGS', raising=False)
	ap = tessphot('aperture', starid, source(), str(tmp_path / 'ap'))
	assert ap.status == STATUS.ERROR and 'edge_flux' in ap._details
	# Halo off (default): today's result
	off = tessphot(None, starid, source(), str(tmp_path / 'off'))
	assert isinstance(off, AperturePhotometry) and off.method == 'aperture'
	assert any('Halo photometry is not available: aperture result kept' in e for e in off._details['errors'])
	# Halo on: the switch runs it
	_settings_on(monkeypatch, tmp_path)
	pho = tessphot(None, starid, source(), str(tmp_path / 'on'))
	assert isinstance(pho, HaloPhotometry) and pho.method == 'halo', pho._details.get('errors')
	assert pho.status == STATUS.OK, pho._details.get('errors')
	assert 'Automatically switched to Halo photometry' in pho._details['errors']
	assert pho._details['edge_flux'] == ap._details['edge_flux']
	hdus = fitsio.read(str(tmp_path / 'on' / pho._details['filepath_lightcurve']))
	assert [h.get('EXTNAME') for h, _ in hdus] == ['PRIMARY', 'LIGHTCURVE', 'SUMIMAGE', 'APERTURE', 'WEIGHTMAP']
	assert hdus[0][0]['PHOTMET'] == 'halo' and hdus[0][0]['NEXTEND'] == 4
