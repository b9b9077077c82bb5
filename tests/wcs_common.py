# -*- coding: utf-8 -*-
"""
A numpy restatement of the TAN-SIP transforms of photometry_amd.wcs / csrc/wcs.hip, in the spherical-trigonometry form of
Calabretta & Greisen (2002, A&A 395, 1077: eqs. 2, 5, 54) and the SIP convention of Shupe et al. (2005, ASP Conf. 347, 491),
with astropy 4.3's ``_all_world2pix`` loop as astropy writes it (vectorised over the batch).  The device works with direction
cosines and a rotation matrix instead; this form checks it.  The header parser is the package's own (host code).
"""
import numpy as np
from photometry_amd.wcs import TanSipWCS

R2D = 180.0 / np.pi


class RefWCS(object):
	def __init__(self, header):
		w = header if isinstance(header, TanSipWCS) else TanSipWCS.from_header(header)
		self.w = w
		self.crpix = w.crpix
		self.ra0, self.dec0 = np.deg2rad(w.crval)
		self.phip = np.deg2rad(w.lonpole)
		self.cd = w.cd
		self.cdinv = np.linalg.inv(w.cd)
		self.has_sip = w.has_sip

	def _sip(self, u, v, coef):
		order, c = coef
		s = np.zeros_like(u)
		for p in range(order + 1):
			for q in range(order + 1 - p):
				if c[p, q] != 0.0:
					s = s + c[p, q] * u**p * v**q
		return s

	def pix2foc(self, pix, origin=0):
		pix = np.asarray(pix, dtype='float64')
		if not self.has_sip:
			return pix.copy()
		x1 = pix[:, 0] + (1 - origin)
		y1 = pix[:, 1] + (1 - origin)
		u, v = x1 - self.crpix[0], y1 - self.crpix[1]
		return np.column_stack((x1 + self._sip(u, v, self.w.a) - (1 - origin), y1 + self._sip(u, v, self.w.b) - (1 - origin)))

	def _foc2world(self, foc, origin):
		d = foc + (1 - origin) - self.crpix
		xy = d @ self.cd.T          # intermediate world coordinates, degrees
		x, y = xy[:, 0], xy[:, 1]
		phi = np.arctan2(x, -y)
		theta = np.arctan2(R2D, np.hypot(x, y))
		dphi = phi - self.phip
		ra = self.ra0 + np.arctan2(-np.cos(theta) * np.sin(dphi), np.sin(theta) * np.cos(self.dec0) - np.cos(theta) * np.sin(self.dec0) * np.cos(dphi))
		dec = np.arcsin(np.sin(theta) * np.sin(self.dec0) + np.cos(theta) * np.cos(self.dec0) * np.cos(dphi))
		return np.column_stack((np.mod(np.rad2deg(ra), 360.0), np.rad2deg(dec)))

	def all_pix2world(self, pix, origin=0):
		return self._foc2world(self.pix2foc(pix, origin), origin)

	def wcs_pix2world(self, pix, origin=0):
		return self._foc2world(np.asarray(pix, dtype='float64'), origin)

	def wcs_world2pix(self, world, origin=0):
		world = np.asarray(world, dtype='float64')
		ra, dec = np.deg2rad(world[:, 0]), np.deg2rad(world[:, 1])
		da = ra - self.ra0
		phi = self.phip + np.arctan2(-np.cos(dec) * np.sin(da), np.sin(dec) * np.cos(self.dec0) - np.cos(dec) * np.sin(self.dec0) * np.cos(da))
		theta = np.arcsin(np.sin(dec) * np.sin(self.dec0) + np.cos(dec) * np.cos(self.dec0) * np.cos(da))
		with np.errstate(divide='ignore', invalid='ignore'):
			r = np.where(theta > 0, R2D / np.tan(theta), np.nan)
		xy = np.column_stack((r * np.sin(phi), -r * np.cos(phi)))
		return xy @ self.cdinv.T + self.crpix - (1 - origin)

	def all_world2pix(self, world, origin=0, tolerance=1e-4, maxiter=20):
		"""astropy 4.3 ``_all_world2pix`` (adaptive=False, detect_divergence=True); returns (pix, k, divergent, slow)."""
		world = np.asarray(world, dtype='float64')
		pix0 = self.wcs_world2pix(world, origin)
		n = len(world)
		if not self.has_sip:
			return pix0, 0, np.zeros(n, bool), np.zeros(n, bool)
		pix = pix0.copy()
		dpix = self.pix2foc(pix, origin) - pix0
		pix -= dpix
		dn = np.sum(dpix * dpix, axis=1)
		dnprev = dn.copy()
		tol2 = tolerance**2
		k = 1
		ind = None
		adaptive = False
		with np.errstate(invalid='ignore', over='ignore'):
			while np.nanmax(dn) >= tol2 and k < maxiter:
				dpix = self.pix2foc(pix, origin) - pix0
				dn = np.sum(dpix * dpix, axis=1)
				divergent = dn >= dnprev
				if np.any(divergent):
					slowconv = dn >= tol2
					if np.any(divergent & slowconv):
						conv = dn < dnprev
						pix[conv] -= dpix[conv]
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
					dpixnew = self.pix2foc(pix[ind], origin) - pix0
					dnnew = np.sum(np.square(dpixnew), axis=1)
					dnprev[ind] = dn[ind].copy()
					dn[ind] = dnnew
					conv = dnnew < dnprev[ind]
					pix[ind[conv]] -= dpixnew[conv]
					subind, = np.where((dnnew >= tol2) & conv)
					ind = ind[subind]
					pix0 = pix0[subind]
					k += 1
			invalid = ~np.all(np.isfinite(pix), axis=1) & np.all(np.isfinite(world), axis=1)
			div = ((dn >= tol2) & (dn >= dnprev)) | invalid
			slow = ((dn >= tol2) & (dn < dnprev) & ~invalid) if k >= maxiter else np.zeros(n, bool)
		return pix, k, div, slow

	def corner_ok(self, maxiter=50):
		"""load_series' test (image_motion.py:300-309): the first calc_footprint(axes=(2, 2)) corner back through all_world2pix."""
		c = self.all_pix2world(np.array([[0.0, 0.0]]), 0)
		_, _, div, slow = self.all_world2pix(c, 0, maxiter=maxiter)
		return not (div.any() or slow.any())


def ra_diff(a, b):
	"""|a - b| of right ascensions in degrees, across the 0 / 360 wrap."""
	d = np.abs(np.asarray(a) - np.asarray(b)) % 360.0
	return np.minimum(d, 360.0 - d)
