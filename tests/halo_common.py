# -*- coding: utf-8 -*-
"""
CPU restatement of Halo photometry (photometry/halo/halo_photometry.py:86-265): the definition the device port
(``photometry_amd/csrc/halo.hip``) and the host layer (``photometry_amd/halo.py``) are held to.  DESIGN.md ("Halo") says the
same in words.

Upstream the numerics come from the third-party ``halophot`` (``do_lc``, :179-196), which is not part of this engine; what is
restated here is the published TV-min method (Pope et al. 2016, MNRAS 455, L36; 2019, ApJS 245, 8) with the reference's settings
(``sub=1, maxiter=101, thresh=-1, minflux=-100, objective='tv', sigclip=False, random_init=False``), written out fully:

* host part -- :func:`pixel_mask`, :func:`split_times`, :func:`segments`, :func:`problems` (the literal :99-173);
* one problem -- :func:`objective`: ``w = softmax(theta)``, ``l = P w`` (float64), ``f = sum |diff(l_F)| / median(l_F)`` and its
  gradient with respect to ``theta``;
* the optimiser -- :func:`lbfgs`: L-BFGS (two-loop recursion, ``H0 = gamma I``) with a backtracking Armijo line search, every
  constant and stopping rule given below;
* the outputs -- :func:`light_curve`, :func:`weightmap`, :func:`flux_err`, and :func:`do_photometry` for a whole target.
"""

import numpy as np

#: TESSQualityFlags.DEFAULT_BITMASK (photometry/quality.py:123-124)
DEFAULT_BITMASK = 1 | 2 | 4 | 8 | 32 | 64 | 128 | 4096
DIST_MAX = 20.0
SETTINGS = {'sub': 1, 'maxiter': 101, 'thresh': -1, 'minflux': -100.0, 'objective': 'tv', 'sigclip': False, 'random_init': False}
#: optimiser constants (scipy's L-BFGS-B ftol / pgtol defaults for the stopping rules)
HISTORY, FTOL, GTOL = 10, 2.220446049250313e-09, 1e-5
C1, MAX_TRIALS, PAIR_CURV = 1e-4, 20, 1e-10
#: problem states (tp_halo_tvmin's d_status)
CONVERGED, CAP_REACHED, LINESEARCH_FAILED, DEGENERATE = 1, 2, 3, 4
#: split times of the sector table (halo_photometry.py:126-133)
SECTOR_SPLITS = {1: (1339., 1347.366, 1349.315), 2: (1368.,), 3: (1395.52,), 8: (1529.50,)}


def mag2flux(mag, zp=20.451):
	return np.clip(10**(-0.4*(mag - zp)), 0, None)


# -- host part ---------------------------------------------------------------------------------------------------------------
def pixel_mask(aperture, stamp, target_row, target_column, dist_max=DIST_MAX):
	"""halo_photometry.py:118-120, with the 1-based pixel grid of get_pixel_grid (BasePhotometry.py:696-706)."""
	cols, rows = np.meshgrid(np.arange(stamp[2] + 1, stamp[3] + 1, 1, dtype='int32'), np.arange(stamp[0] + 1, stamp[1] + 1, 1, dtype='int32'))
	dist = np.sqrt((cols - target_column)**2 + (rows - target_row)**2)
	return (np.asarray(aperture) & 1 != 0) & (dist <= dist_max)


def split_times(sector, time, timecorr):
	"""halo_photometry.py:110, :125-159: the split times, or None.  ``time`` / ``timecorr`` of every cadence."""
	good = np.isfinite(time)
	t_good = np.asarray(time)[good]
	if sector in SECTOR_SPLITS:
		st = SECTOR_SPLITS[sector]
	else:
		tc = np.asarray(timecorr)[good]
		t = t_good - tc
		dt = np.append(np.diff(t), 0)
		t0 = np.nanmin(t)
		Ttot = np.nanmax(t) - t0
		indx = (t0 + 0.30*Ttot < t) & (t < t0 + 0.70*Ttot) & (dt > 0.5)
		if np.sum(indx) == 1:
			i = np.where(indx)[0][0]
			st = (0.5*(t[i] + t[i+1]) + tc[i],)
		else:
			st = None
	if st is not None:
		st = tuple([s for s in st if np.min(t_good) < s < np.max(t_good)])
		if not st:
			st = None
	return st


def segments(time, splits):
	"""Segment of every cadence: ``searchsorted(split_times, time, 'right')`` (-1 for a cadence without a finite time)."""
	time = np.asarray(time)
	seg = np.full(len(time), -1, dtype='int64')
	good = np.isfinite(time)
	seg[good] = np.searchsorted(np.asarray(splits if splits else (), dtype='float64'), time[good], side='right')
	return seg


def problems(images, quality, mask, seg, minflux=SETTINGS['minflux']):
	"""
	The problems of one target.  ``images`` (rows, cols, T) float32, ``mask`` the pixel mask, ``seg`` from :func:`segments`.
	Per segment k (in order): a dict with ``pix`` (flat indices into the stamp of the pixels kept), ``cad`` (cadences of the
	problem: good time, segment k, every kept pixel finite), ``P`` float32 (len(cad), len(pix)) and ``fit`` bool.
	"""
	R, C, T = images.shape
	flat = images.reshape(R * C, T)
	mpix = np.flatnonzero(np.asarray(mask).ravel())
	quality = np.asarray(quality)
	out = []
	for k in range(int(seg.max()) + 1 if len(seg) and seg.max() >= 0 else 0):
		c_all = np.flatnonzero(seg == k)
		fitq = (quality[c_all] & DEFAULT_BITMASK) == 0
		# minflux: the median over the fitted cadences of the segment of every mask pixel
		with np.errstate(all='ignore'):
			import warnings
			with warnings.catch_warnings():
				warnings.simplefilter('ignore', RuntimeWarning)
				med = np.nanmedian(flat[np.ix_(mpix, c_all[fitq])].astype('float64'), axis=1) if fitq.any() else np.full(len(mpix), np.nan)
		pix = mpix[~(med < minflux)]
		fin = np.all(np.isfinite(flat[np.ix_(pix, c_all)]), axis=0) if len(pix) else np.ones(len(c_all), bool)
		cad = c_all[fin]
		P = np.ascontiguousarray(flat[np.ix_(pix, cad)].T).astype('float32')
		out.append({'pix': pix, 'cad': cad, 'P': P, 'fit': (quality[cad] & DEFAULT_BITMASK) == 0})
	return out


# -- one problem -------------------------------------------------------------------------------------------------------------
def softmax(theta):
	e = np.exp(theta - np.max(theta))
	return e / np.sum(e)


def objective(P, fit, theta, with_grad=True):
	"""
	``f`` and ``grad_theta`` (NaN for a degenerate problem).  ``P`` float32 (ncad, npix), ``fit`` bool (ncad,).
	Gradient with respect to w: ``g_p = sum_t P[t,p] s_t / m - (f / m) P[t_med, p]`` with ``s_t = sign(D_t-1) - sign(D_t)``
	(differences of consecutive fitted l), ``t_med`` the cadence of the median (stable order; the mean of the two middle rows for
	an even count); through the softmax: ``w (g - w.g)``.
	"""
	P = np.asarray(P)
	F = np.flatnonzero(fit)
	nf = len(F)
	theta = np.asarray(theta, dtype='float64')
	nan = (np.nan, np.full(len(theta), np.nan)) if with_grad else np.nan
	if nf < 3:
		return nan
	w = softmax(theta)
	PF = P[F].astype('float64')
	lF = PF @ w
	m = np.median(lF)
	if not (np.isfinite(m) and m > 0):
		return nan
	dl = np.diff(lF)
	f = np.sum(np.abs(dl)) / m
	if not with_grad:
		return f
	sg = np.sign(dl)
	s = np.zeros(nf)
	s[1:] += sg
	s[:-1] -= sg
	order = np.argsort(lF, kind='stable')
	if nf % 2:
		pm = PF[order[nf // 2]]
	else:
		pm = (PF[order[nf // 2 - 1]] + PF[order[nf // 2]]) * 0.5
	g = (s @ PF) / m - (f / m) * pm
	return f, w * (g - w @ g)


def lbfgs(P, fit, maxiter=SETTINGS['maxiter'], history=HISTORY, ftol=FTOL, gtol=GTOL, theta0=None, trace=None):
	"""
	The optimiser of tp_halo_tvmin.  From ``theta = 0``: gradient ``g``; if ``|g|_inf <= gtol`` converged (0 iterations).
	Iteration: direction ``d`` by the two-loop recursion over the stored pairs (oldest .. newest, ``gamma = s.y / y.y`` of the
	newest), ``-g / |g|_2`` without pairs or when ``g.d >= 0`` (the pairs are then dropped); line search ``alpha = 1, 1/2, ...``
	(at most 20 trials) until ``f(theta + alpha d) <= f + 1e-4 alpha g.d`` (a trial with a median <= 0 fails), else status 3 with
	theta kept; accepted: ``s = theta_new - theta``, ``y = g_new - g``, the pair kept (the oldest of ``history`` dropped) if
	``s.y > 1e-10 y.y``; then in order: ``f_k - f_k+1 <= ftol max(|f_k|, |f_k+1|, 1)`` -> 1, ``|g_new|_inf <= gtol`` -> 1,
	``iterations >= maxiter`` -> 2.  Returns dict ``theta, w, f, iterations, status``.

	``trace`` (a dict, optional) only records what was decided: ``trials`` gets ``(fn, f + C1 alpha g.d, accepted)`` of every
	line-search trial, ``pairs`` gets ``(s.y, 1e-10 y.y, kept)`` of every accepted step, ``stops`` gets
	``(f_k - f_k+1, ftol max(|f_k|, |f_k+1|, 1), |g_new|_inf)`` of every accepted step.
	"""
	n = P.shape[1]
	theta = np.zeros(n) if theta0 is None else np.asarray(theta0, dtype='float64').copy()
	f, g = objective(P, fit, theta)
	if not np.isfinite(f):
		return {'theta': theta, 'w': softmax(theta), 'f': np.nan, 'iterations': 0, 'status': DEGENERATE}
	S, Y, SY, YY = [], [], [], []
	it = 0
	if np.max(np.abs(g)) <= gtol:
		return {'theta': theta, 'w': softmax(theta), 'f': f, 'iterations': 0, 'status': CONVERGED}
	if maxiter <= 0:
		return {'theta': theta, 'w': softmax(theta), 'f': f, 'iterations': 0, 'status': CAP_REACHED}
	while True:
		d = None
		if S:
			q = g.copy()
			a = [0.0] * len(S)
			for i in range(len(S) - 1, -1, -1):
				a[i] = (1.0 / SY[i]) * (S[i] @ q)
				q = q - a[i] * Y[i]
			r = (SY[-1] / YY[-1]) * q
			for i in range(len(S)):
				b = (1.0 / SY[i]) * (Y[i] @ r)
				r = r + S[i] * (a[i] - b)
			d = -r
			gtd = g @ d
			if not gtd < 0:
				S, Y, SY, YY = [], [], [], []
				d = None
		if d is None:
			d = -g / np.sqrt(g @ g)
			gtd = g @ d
		alpha = 1.0
		for trial in range(MAX_TRIALS):
			tn = theta + alpha * d
			fn = objective(P, fit, tn, with_grad=False)
			accepted = bool(np.isfinite(fn) and fn <= f + C1 * alpha * gtd)
			if trace is not None:
				trace.setdefault('trials', []).append((float(fn), float(f + C1 * alpha * gtd), accepted))
			if accepted:
				break
			alpha = alpha * 0.5
		else:
			return {'theta': theta, 'w': softmax(theta), 'f': f, 'iterations': it, 'status': LINESEARCH_FAILED}
		it += 1
		fn, gn = objective(P, fit, tn)
		s, y = tn - theta, gn - g
		sy, yy = s @ y, y @ y
		if trace is not None:
			trace.setdefault('pairs', []).append((float(sy), float(PAIR_CURV * yy), bool(sy > PAIR_CURV * yy)))
			trace.setdefault('stops', []).append((float(f - fn), float(ftol * max(abs(f), abs(fn), 1.0)), float(np.max(np.abs(gn)))))
		if sy > PAIR_CURV * yy:
			S.append(s); Y.append(y); SY.append(sy); YY.append(yy)
			if len(S) > history:
				S.pop(0); Y.pop(0); SY.pop(0); YY.pop(0)
		f_old, theta, f, g = f, tn, fn, gn
		if f_old - f <= ftol * max(abs(f_old), abs(f), 1.0):
			status = CONVERGED
		elif np.max(np.abs(g)) <= gtol:
			status = CONVERGED
		elif it >= maxiter:
			status = CAP_REACHED
		else:
			continue
		return {'theta': theta, 'w': softmax(theta), 'f': f, 'iterations': it, 'status': status}


def light_curve(P, fit, w):
	"""``l`` at every cadence of the problem and the median over the fitted ones."""
	lc = np.asarray(P).astype('float64') @ w
	return lc, np.median(lc[np.asarray(fit, bool)])


# -- outputs -----------------------------------------------------------------------------------------------------------------
def weightmap(shape, pix, w, median):
	"""``w / median(l)`` placed into the stamp, zero elsewhere: ``sum(wm * image) = corr_flux`` at every cadence."""
	wm = np.zeros(int(np.prod(shape)))
	wm[pix] = w / median
	return wm.reshape(shape)


def flux_err(weightmaps, seg, images_err, tmag):
	"""halo_photometry.py:210-219 with the weight map of the segment of every cadence; 0 where the time is not finite."""
	out = np.zeros(images_err.shape[2])
	nf = np.abs(mag2flux(tmag))
	for k in range(images_err.shape[2]):
		if seg[k] < 0:
			continue
		out[k] = nf * np.sqrt(np.nansum(weightmaps[seg[k]]**2 * images_err[:, :, k].astype('float64')**2))
	return out


def do_photometry(images, images_err, quality, time, timecorr, aperture, stamp, target_row, target_column, tmag, sector):
	"""The whole CPU restatement for one target: dict with ``flux``, ``corr_flux``, ``flux_err``, ``weightmaps``, ``mask``, ``fits``."""
	mask = pixel_mask(aperture, stamp, target_row, target_column)
	splits = split_times(sector, time, timecorr)
	seg = segments(time, splits)
	T = images.shape[2]
	corr = np.full(T, np.nan)
	wms, fits = [], []
	for pr in problems(images, quality, mask, seg):
		res = lbfgs(pr['P'], pr['fit'])
		lc, med = light_curve(pr['P'], pr['fit'], res['w'])
		corr[pr['cad']] = lc / med
		wms.append(weightmap(images.shape[:2], pr['pix'], res['w'], med))
		fits.append(res)
	return {'corr_flux': corr, 'flux': corr * mag2flux(tmag), 'flux_err': flux_err(wms, seg, images_err, tmag), 'weightmaps': wms,
		'mask': mask, 'fits': fits, 'segments': seg, 'split_times': splits}


# -- synthetic known-answer scene -----------------------------------------------------------------------------------------------
def bright_star_scene(seed=7, T=480, R=44, C=44, row0=300, col0=500, tmag=5.0, amplitude=1e-3, period=5.0, sat_level=6e4,
	gain_sigma=0.02, step=0.02, t0=1363.0, noise_scale=1800.0):
	"""
	A saturated ``Tmag 5`` star with a bleed column (the charge above ``sat_level`` spread up and down its column), +-2 % pixel gain
	errors, a sub-pixel pointing random walk (the same jitter moves the star in the images and is handed over as ``pos_corr``)
	and an injected sinusoid, at 30-min cadence around the sector-2 split (1368.0).  Images in electrons per second with the photon
	noise of ``noise_scale`` seconds of exposure.  Returns a dict of what a
	``MemoryStampSource`` takes plus the truth (``signal``, ``jitter``).
	"""
	from scipy.special import erf
	rng = np.random.default_rng(seed)
	time = t0 + np.arange(T) * 1800.0 / 86400.0
	signal = amplitude * np.sin(2 * np.pi * time / period)
	jitter = np.clip(np.cumsum(rng.normal(scale=step, size=(T, 2)), axis=0), -0.4, 0.4)   # (column, row)
	r_star, c_star = row0 + R / 2 + 0.3, col0 + C / 2 - 0.4
	gain = 1.0 + gain_sigma * rng.uniform(-1, 1, size=(R, C))
	flux = mag2flux(tmag)
	rr, cc = np.arange(R) + row0, np.arange(C) + col0
	sig = 1.0
	images = np.empty((R, C, T), dtype='float64')
	for k in range(T):
		r, c = r_star + jitter[k, 1], c_star + jitter[k, 0]
		pr = 0.5 * (erf((rr + 0.5 - r) / (np.sqrt(2) * sig)) - erf((rr - 0.5 - r) / (np.sqrt(2) * sig)))
		pc = 0.5 * (erf((cc + 0.5 - c) / (np.sqrt(2) * sig)) - erf((cc - 0.5 - c) / (np.sqrt(2) * sig)))
		img = flux * (1.0 + signal[k]) * np.outer(pr, pc)
		# bleed: the charge of a column above the full well fills the pixels next to the peak, alternately below and above
		for j in np.flatnonzero(img.max(axis=0) > sat_level):
			col = img[:, j]
			excess = np.sum(np.clip(col - sat_level, 0, None))
			i = int(np.argmax(col))
			col = np.minimum(col, sat_level)
			up, dn, turn = i - 1, i + 1, 0
			while excess > 0 and (up >= 0 or dn < R):
				idx = dn if (turn == 0 and dn < R) or up < 0 else up
				take = min(max(sat_level - col[idx], 0.0), excess)
				col[idx] += take
				excess -= take
				if idx == dn:
					dn += 1
				else:
					up -= 1
				turn ^= 1
			img[:, j] = col
		images[:, :, k] = img * gain
	bkg = 200.0
	noise = np.sqrt((np.abs(images) + bkg) / noise_scale)
	images = images + rng.normal(size=images.shape) * noise
	quality = np.zeros(T, dtype='int32')
	quality[rng.choice(T, size=T // 50, replace=False)] = 32
	cat = {'starid': np.array([7, 8], dtype='int64'), 'tmag': np.array([tmag, 13.0], dtype='float32'),
		'row': np.array([r_star, row0 + 5.2], dtype='float32'), 'column': np.array([c_star, col0 + 6.1], dtype='float32')}
	targets = {'starid': cat['starid'].copy(), 'tmag': np.array([tmag, 13.0]), 'row': np.array([r_star, row0 + 5.2]),
		'column': np.array([c_star, col0 + 6.1])}
	frames = {'images': images.astype('float32'), 'images_err': noise.astype('float32'), 'backgrounds': np.full(images.shape, bkg, dtype='float32')}
	return {'frames': frames, 'row0': row0, 'col0': col0, 'time': time, 'timecorr': np.zeros(T), 'cadenceno': np.arange(T) + 1000,
		'quality': quality, 'catalog': cat, 'targets': targets, 'jitter': jitter, 'signal': signal, 'period': period, 'starid': 7}


def sinusoid_fit(time, y, seg, period):
	"""Least-squares amplitude of ``sin / cos`` at ``period`` with one offset per segment, and the rms of the residual."""
	ok = np.isfinite(y) & (seg >= 0)
	cols = [np.sin(2 * np.pi * time[ok] / period), np.cos(2 * np.pi * time[ok] / period)]
	for k in np.unique(seg[ok]):
		cols.append((seg[ok] == k).astype(float))
	A = np.column_stack(cols)
	coef, *_ = np.linalg.lstsq(A, y[ok], rcond=None)
	return float(np.hypot(coef[0], coef[1])), float(np.std(y[ok] - A @ coef))
