#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Generator of ``golden_wcs.npz``: astropy.wcs (4.3, wcslib) and the reference's ``ImageMovementKernel(warpmode='wcs')``
(photometry/image_motion.py:113-421) on TESS-like TAN-SIP headers.

Recorded per header (``hdr_<i>_*``): ``all_pix2world`` / ``wcs_pix2world`` / ``pix2foc`` of a pixel grid and of random pixels,
``all_world2pix`` (default tolerance and maxiter, ``quiet=True``) / ``wcs_world2pix`` of the grid's world points (one batch)
and of random world points (a second batch), with astropy's iteration count per batch and its divergent / slow-convergence
points from an instrumented copy of ``_all_world2pix`` (checked equal to astropy's own result), and ``calc_footprint``.
Recorded for a series of drifting frames (``series_*``): the frames ``load_series`` keeps, ``interpolate`` at hits, between
frames, in the end margins and outside (``ValueError``), and ``jitter``.

Run with a Python that has astropy 4.3 (numpy shims below), the reference checkout named by ``TESSPHOT_REFERENCE``:
``TESSPHOT_REFERENCE=<checkout> python3.9 tests/golden/make_golden_wcs.py``.  cv2 and skimage are stubbed (the 'wcs' warpmode
does not use them); astropy is the real one.  The result is committed.
"""

import os
import sys
import types
import numpy as np

np.asscalar = lambda a: a.item()
np.alen = len
for name in ('cv2', 'skimage', 'skimage.filters'):
	sys.modules[name] = types.ModuleType(name)
sys.modules['skimage'].filters = sys.modules['skimage.filters']
sys.modules['skimage.filters'].scharr = None

from astropy.io import fits # noqa: E402
from astropy.wcs import WCS, NoConvergence # noqa: E402

sys.path.insert(0, os.environ['TESSPHOT_REFERENCE'])
sys.modules['photometry'] = types.ModuleType('photometry')
sys.modules['photometry'].__path__ = [os.path.join(os.environ['TESSPHOT_REFERENCE'], 'photometry')]
from photometry.image_motion import ImageMovementKernel # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NAXIS = (2136, 2078)


def tess_header(rng, ra, dec, order, rot_deg=0.0, pc=False, scale=1.0, alt=True, dexp=False, lonpole=None):
	h = fits.Header()
	h['WCSAXES'] = 2
	h['NAXIS1'], h['NAXIS2'] = NAXIS
	h['CTYPE1'] = 'RA---TAN-SIP' if order else 'RA---TAN'
	h['CTYPE2'] = 'DEC--TAN-SIP' if order else 'DEC--TAN'
	h['CUNIT1'] = h['CUNIT2'] = 'deg'
	h['CRPIX1'] = 1045.0 + rng.uniform(-20, 20)
	h['CRPIX2'] = 1001.0 + rng.uniform(-20, 20)
	h['CRVAL1'] = ra
	h['CRVAL2'] = dec
	s = 21.0 / 3600.0
	c, sn = np.cos(np.deg2rad(rot_deg)), np.sin(np.deg2rad(rot_deg))
	cd = s * np.array([[-c, sn], [sn, c]]) * (1 + rng.normal(0, 1e-3, (2, 2)))
	if pc:
		h['CDELT1'], h['CDELT2'] = -s, s
		h['PC1_1'], h['PC1_2'], h['PC2_1'], h['PC2_2'] = cd[0, 0] / -s, cd[0, 1] / -s, cd[1, 0] / s, cd[1, 1] / s
	else:
		h['CD1_1'], h['CD1_2'], h['CD2_1'], h['CD2_2'] = cd.ravel()
	if lonpole is not None:
		h['LONPOLE'] = lonpole
	h['RADESYS'] = 'ICRS'
	if order:
		h['A_ORDER'] = h['B_ORDER'] = order
		for p in range(order + 1):
			for q in range(order + 1 - p):
				if p + q >= 2:
					h[f'A_{p}_{q}'] = scale * rng.normal(0, 2.0) / 1000.0 ** (p + q)
					h[f'B_{p}_{q}'] = scale * rng.normal(0, 2.0) / 1000.0 ** (p + q)
		# the largest distortion, as TESS and other SIP headers record it (astropy ignores these two cards)
		h['A_DMAX'] = 44.72893589844534
		h['B_DMAX'] = 44.62692873032506
		h['AP_ORDER'] = h['BP_ORDER'] = order
		for p in range(order + 1):
			for q in range(order + 1 - p):
				h[f'AP_{p}_{q}'] = -h.get(f'A_{p}_{q}', 0.0)
				h[f'BP_{p}_{q}'] = -h.get(f'B_{p}_{q}', 0.0)
	if alt:
		h['WCSNAMEP'] = 'PHYSICAL'
		h['CTYPE1P'] = 'RAWX'
		h['CTYPE2P'] = 'RAWY'
		h['CRPIX1P'] = 1.0
		h['CRVAL1P'] = 45.0
	h.add_comment('a TESS-like test header')
	s = h.tostring()
	if dexp:
		s = s.replace("E-", "D-", 3)
	return s


def instrumented(w, world, origin=0, tolerance=1e-4, maxiter=20):
	"""astropy 4.3 _all_world2pix (adaptive=False, detect_divergence=True) with its iteration count k and flagged points."""
	pix0 = w.wcs_world2pix(world, origin)
	if not w.has_distortion:
		return pix0, 0, np.zeros(len(world), bool), np.zeros(len(world), bool)
	pix = pix0.copy()
	dpix = w.pix2foc(pix, origin) - pix0
	pix -= dpix
	dn = np.sum(dpix * dpix, axis=1)
	dnprev = dn.copy()
	tol2 = tolerance**2
	k = 1
	ind = None
	adaptive = False
	with np.errstate(invalid='ignore', over='ignore'):
		while np.nanmax(dn) >= tol2 and k < maxiter:
			dpix = w.pix2foc(pix, origin) - pix0
			dn = np.sum(dpix * dpix, axis=1)
			divergent = (dn >= dnprev)
			if np.any(divergent):
				slowconv = (dn >= tol2)
				inddiv, = np.where(divergent & slowconv)
				if inddiv.shape[0] > 0:
					conv = (dn < dnprev)
					iconv = np.where(conv)
					dpixgood = dpix[iconv]
					pix[iconv] -= dpixgood
					dpix[iconv] = dpixgood
					ind, = np.where(slowconv & conv)
					pix0 = pix0[ind]
					dnprev[ind] = dn[ind]
					k += 1
					adaptive = True
					break
			dnprev = dn
			pix -= dpix
			k += 1
		if adaptive:
			while ind.shape[0] > 0 and k < maxiter:
				dpixnew = w.pix2foc(pix[ind], origin) - pix0
				dnnew = np.sum(np.square(dpixnew), axis=1)
				dnprev[ind] = dn[ind].copy()
				dn[ind] = dnnew
				conv = (dnnew < dnprev[ind])
				iconv = np.where(conv)
				iiconv = ind[iconv]
				dpixgood = dpixnew[iconv]
				pix[iiconv] -= dpixgood
				dpix[iiconv] = dpixgood
				subind, = np.where((dnnew >= tol2) & conv)
				ind = ind[subind]
				pix0 = pix0[subind]
				k += 1
		invalid = ((~np.all(np.isfinite(pix), axis=1)) & (np.all(np.isfinite(world), axis=1)))
		div = ((dn >= tol2) & (dn >= dnprev)) | invalid
		slow = (dn >= tol2) & (dn < dnprev) & ~invalid if k >= maxiter else np.zeros(len(world), bool)
	return pix, k, div, slow


def main():
	rng = np.random.default_rng(20261016)
	out = {}
	hdrs = [
		('order2', tess_header(rng, 84.1, -62.3, 2, rot_deg=12.0)),
		('order3', tess_header(rng, 301.7, 45.2, 3, rot_deg=-170.0)),
		('order4', tess_header(rng, 12.5, -20.0, 4, rot_deg=95.0, dexp=True)),
		('order5', tess_header(rng, 359.99, 5.0, 5, rot_deg=45.0)),
		('order6', tess_header(rng, 180.0, 75.0, 6, rot_deg=-30.0)),
		('pc_cdelt', tess_header(rng, 250.3, -35.0, 4, rot_deg=3.0, pc=True)),
		('nosip', tess_header(rng, 120.0, 10.0, 0, rot_deg=20.0, alt=False)),
		('lonpole', tess_header(rng, 60.0, -80.0, 3, rot_deg=0.0, lonpole=170.0)),
		('divergent', tess_header(rng, 30.0, 30.0, 2, scale=3000.0)),
	]
	out['hdr_names'] = np.array([n for n, _ in hdrs])
	out['hdr_strings'] = np.array([s for _, s in hdrs])
	gx, gy = np.meshgrid(np.linspace(-50, NAXIS[0] + 50, 13), np.linspace(-50, NAXIS[1] + 50, 11))
	for i, (name, s) in enumerate(hdrs):
		w = WCS(fits.Header.fromstring(s), relax=True)
		grid = np.column_stack((gx.ravel(), gy.ravel()))
		rnd = np.column_stack((rng.uniform(0, NAXIS[0], 60), rng.uniform(0, NAXIS[1], 60)))
		pts = np.concatenate((grid, rnd))
		out[f'hdr_{i}_pix'] = pts
		out[f'hdr_{i}_all_pix2world'] = w.all_pix2world(pts, 0)
		out[f'hdr_{i}_all_pix2world_o1'] = w.all_pix2world(pts, 1)
		out[f'hdr_{i}_wcs_pix2world'] = w.wcs_pix2world(pts, 0)
		out[f'hdr_{i}_pix2foc'] = w.pix2foc(pts, 0)
		out[f'hdr_{i}_footprint'] = w.calc_footprint(axes=NAXIS)
		out[f'hdr_{i}_footprint22'] = w.calc_footprint(axes=(2, 2))
		# world batches: the grid's world points, and random points around the field
		wgrid = w.all_pix2world(grid, 0)
		wrnd = w.all_pix2world(rnd, 0) + rng.normal(0, 0.05, rnd.shape)
		for b, world in enumerate((wgrid, wrnd)):
			mine, k, div, slow = instrumented(w, world)
			ref = w.all_world2pix(world, 0, quiet=True)
			assert np.array_equal(mine, ref, equal_nan=True), name
			out[f'hdr_{i}_world{b}'] = world
			out[f'hdr_{i}_all_world2pix{b}'] = ref
			out[f'hdr_{i}_wcs_world2pix{b}'] = w.wcs_world2pix(world, 0)
			out[f'hdr_{i}_iters{b}'] = np.int32(k)
			out[f'hdr_{i}_divergent{b}'] = div
			out[f'hdr_{i}_slow{b}'] = slow
		try:
			w.all_world2pix(np.atleast_2d(w.calc_footprint(axes=(2, 2))[0]), 0, maxiter=50)
			out[f'hdr_{i}_corner_ok'] = True
		except (NoConvergence, ValueError):
			out[f'hdr_{i}_corner_ok'] = False

	# a drifting series: CRVAL by arcseconds, CD rotated by arcseconds, one blank header, one whose corner diverges
	T = 40
	times = 1500.0 + np.arange(T) * 0.0208333 + rng.normal(0, 1e-4, T)
	base = fits.Header.fromstring(hdrs[2][1])
	series = []
	for k in range(T):
		h = base.copy()
		h['CRVAL1'] = base['CRVAL1'] + 2.0 / 3600 * np.sin(k / 6.0)
		h['CRVAL2'] = base['CRVAL2'] + 1.5 / 3600 * np.cos(k / 5.0)
		a = np.deg2rad(3.0 / 3600 * np.sin(k / 4.0) * 50)
		cd = np.array([[base['CD1_1'], base['CD1_2']], [base['CD2_1'], base['CD2_2']]])
		cd = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) @ cd
		h['CD1_1'], h['CD1_2'], h['CD2_1'], h['CD2_2'] = cd.ravel()
		series.append(h.tostring())
	series[7] = ' ' * 80
	series[23] = hdrs[-1][1]
	ref_hdr = series[0]
	out['series_times'] = times
	out['series_headers'] = np.array(series)
	out['series_ref'] = ref_hdr
	imk = ImageMovementKernel(warpmode='wcs', wcs_ref=WCS(fits.Header.fromstring(ref_hdr), relax=True))
	imk.load_series(times, list(series))
	out['series_kept'] = np.isin(times, imk.series_times)
	xy = np.array([[100.5, 200.25], [1500.0, 30.0], [1000.0, 1000.0], [2100.0, 2050.0], [-3.0, 5.0]])
	kept = imk.series_times
	dtm = np.median(np.diff(kept))
	q = np.concatenate((kept[[0, 3, 10, 30, -1]], 0.5 * (kept[4:8] + kept[5:9]), kept[[12, 20]] + 0.3 * dtm,
		[kept[0] - 0.5 * dtm, kept[-1] + 0.7 * dtm]))
	out['series_xy'] = xy
	out['series_query'] = q
	out['series_interpolate'] = np.array([imk.interpolate(t, xy) for t in q])
	bad = np.array([kept[0] - 1.5 * dtm, kept[-1] + 2.0 * dtm])
	for t in bad:
		try:
			imk.interpolate(t, xy)
			raise AssertionError("no error")
		except ValueError:
			pass
	out['series_bad_query'] = bad
	jt = np.concatenate((kept[:: 3], 0.5 * (kept[1:6] + kept[2:7])))
	out['series_jitter_time'] = jt
	out['series_jitter_at'] = np.array([812.3, 640.7])
	out['series_jitter'] = imk.jitter(jt, 812.3, 640.7)
	np.savez_compressed(os.path.join(HERE, 'golden_wcs.npz'), **out)
	print("kept", out['series_kept'].sum(), "of", T, "; iterations", [int(out[f'hdr_{i}_iters{b}']) for i in range(len(hdrs)) for b in (0, 1)])


if __name__ == '__main__':
	main()
