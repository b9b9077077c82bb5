# -*- coding: utf-8 -*-
"""
The PSFPhotometry flux errors through the plugin and the batched frames entry: with ``[psf] flux_errors = true`` in the
settings ``tessphot('psf')`` ends OK with diagnostics and a light-curve file whose FLUX_RAW_ERR is the restatement of the definition
(``tests/psf_err_common.py``) at the fit's own end points; with the switch off nothing differs from the reference's behaviour
(STATUS.ERROR, psf_photometry.py:175); ``psf_frames(..., flux_errors=True)`` fills ``flux_err`` with the plugin's bits and changes
nothing else.
"""
import os
import numpy as np
import pytest
import psf_err_common as pe

pytestmark = pytest.mark.gpu


@pytest.fixture()
def settings_on(tmp_path):
	"""A settings file that turns the switch on, named by TESSPHOT_SETTINGS; the variable is restored afterwards."""
	f = tmp_path / 'settings.ini'
	f.write_text('[psf]\nflux_errors = true\n')
	old = os.environ.get('TESSPHOT_SETTINGS')

	def switch(on):
		if on:
			os.environ['TESSPHOT_SETTINGS'] = str(f)
		else:
			os.environ.pop('TESSPHOT_SETTINGS', None)
	yield switch
	if old is None:
		os.environ.pop('TESSPHOT_SETTINGS', None)
	else:
		os.environ['TESSPHOT_SETTINGS'] = old


def _restate_plugin(pho, prf, images, backgrounds, images_err):
	"""The restatement at the parameters the plugin's fit ended on (``pho.psf_params``), with its stamp, mini aperture and variance floor."""
	from oracle import psf as opsf
	p = opsf.PSF(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'], tuple(pho.stamp))
	floor = pho.n_readout * pho.readnoise**2 / pho.gain**2
	return pe.flux_err_series(p, images, backgrounds, images_err, pho.psf_params, pho._minimum_aperture(), var_floor=floor, cutoff_radius=pho.cutoff_radius)


def test_tessphot_psf_with_flux_errors(tmp_path, settings_on):
	from photometry_amd import STATUS, tessphot, simulate, fitsio, psf as hpsf
	from photometry_amd.device import Context
	from photometry_amd.source import source_from_scene
	from oracle import psf as opsf
	s = simulate.make_scene(2, 4, 11, 11, seed=71, max_neighbours=1, neighbour_tmag_range=(9.0, 14.0))
	simulate.fill_cubes(s, nan_fraction=0.003)
	prf = opsf.synthetic_prf(seed=4)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	ctx = Context(0)
	try:
		def run(on, i, out):
			settings_on(on)
			src = source_from_scene(s, i)
			src.prf = model
			os.makedirs(out, exist_ok=True)
			return tessphot('psf', int(s.target_starid[i]), src, out, ctx=ctx)
		for i in range(2):
			on = run(True, i, str(tmp_path / f'on{i}'))
			assert on.method == 'psf' and on.status == STATUS.OK, on._details.get('errors')
			for key in ('mean_flux', 'variance', 'rms_hour', 'ptp'):
				assert key in on._details
			assert on.additional_headers['PSF_FERR'][0] is True
			ref = _restate_plugin(on, prf, s.images[i], s.backgrounds[i], s.images_err[i])
			fin = np.isfinite(on.lightcurve['flux'])
			assert fin.sum() >= 2
			np.testing.assert_array_equal(np.isnan(ref), ~fin)      # NaN exactly where the fit did not finish
			pe.assert_flux_err(on.lightcurve['flux_err'], ref, label=f'plugin flux_err target {i}')
			assert np.all(on.lightcurve['flux_err'][fin] > 0)
			fname = os.path.join(str(tmp_path / f'on{i}'), on._details['filepath_lightcurve'])
			assert os.path.exists(fname)
			hdus = fitsio.read(fname)
			np.testing.assert_array_equal(hdus[1][1]['FLUX_RAW_ERR'], on.lightcurve['flux_err'])
			assert np.isfinite(hdus[1][1]['FLUX_RAW_ERR']).sum() >= 2
			assert hdus[0][0]['PSF_FERR'] is True or hdus[0][0]['PSF_FERR'] == 1
			off = run(False, i, str(tmp_path / f'off{i}'))
			assert off.status == STATUS.ERROR and any('errors are all NaNs' in e for e in off._details['errors'])
			assert 'PSF_FERR' not in off.additional_headers and np.all(np.isnan(off.lightcurve['flux_err']))
			np.testing.assert_array_equal(off.lightcurve['flux'], on.lightcurve['flux'])
			np.testing.assert_array_equal(off.lightcurve['pos_centroid'], on.lightcurve['pos_centroid'])
	finally:
		ctx.close()


def test_psf_frames_with_flux_errors(tmp_path, settings_on):
	from test_gpu_psf_frames import _region
	from photometry_amd import pipeline, psf as hpsf, simulate
	from photometry_amd.device import Context
	from photometry_amd.plugins import PSFPhotometry
	from photometry_amd.source import MemoryStampSource
	T = 4
	frames, row0, col0, time, quality, cat, targets, jitter = _region(T=T)
	# four targets, two stamp sizes: the brightest star's default stamp is larger than the others'
	keep = np.array([0, 2, 5, 7])
	targets = {k: v[keep] for k, v in targets.items()}
	prf = simulate.synthetic_prf(seed=3)
	model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
	ctx = Context(0)
	try:
		stack = pipeline.FrameStack(ctx, {k: np.moveaxis(v, 2, 0) for k, v in frames.items()}, row0, col0)
		src = MemoryStampSource(frames, row0, col0, time, np.zeros(T), np.arange(T), quality, cat, targets=targets, jitter=jitter, prf=model)
		kw = dict(readnoise=10, gain=100, n_readout=src.n_readout)
		plain = pipeline.psf_frames(ctx, stack, targets, cat, time, quality, model, **kw)
		with_err = pipeline.psf_frames(ctx, stack, targets, cat, time, quality, model, flux_errors=True, **kw)
		assert np.all(np.isnan(plain.flux_err))
		np.testing.assert_array_equal(with_err.flux, plain.flux)
		np.testing.assert_array_equal(with_err.pos_centroid, plain.pos_centroid)
		np.testing.assert_array_equal(with_err.status, plain.status)
		np.testing.assert_array_equal(with_err.stamp, plain.stamp)
		assert len({(st[1] - st[0], st[3] - st[2]) for st in with_err.stamp.tolist()}) >= 2
		np.testing.assert_array_equal(np.isnan(with_err.flux_err), np.isnan(with_err.flux))
		assert np.isfinite(with_err.flux_err).sum() >= 2 * len(keep)
		settings_on(True)
		for i in range(len(keep)):
			with PSFPhotometry(int(targets['starid'][i]), src, str(tmp_path), ctx=ctx) as pho:
				pho.do_photometry()
				assert tuple(pho.stamp) == with_err[i]['stamp']
				np.testing.assert_array_equal(pho.lightcurve['flux'], with_err.flux[i])
				np.testing.assert_array_equal(pho.lightcurve['flux_err'], with_err.flux_err[i])      # the plugin's, bit for bit
				if i == 1:
					st = pho.stamp
					cut = {k: v[st[0] - row0:st[1] - row0, st[2] - col0:st[3] - col0, :] for k, v in frames.items()}
					pe.assert_flux_err(with_err.flux_err[i], _restate_plugin(pho, prf, cut['images'], cut['backgrounds'], cut['images_err']), label='frames target 1')
	finally:
		ctx.close()
