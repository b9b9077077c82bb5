# -*- coding: utf-8 -*-
"""
The CCD region the batched Halo tests run on (tests/test_halo_frames_host.py proves its properties on the oracle alone,
tests/test_gpu_halo_frames.py runs it on the device): faint stars, three Tmag < 6 stars whose bleed trails run into three different
frame limits (their aperture runs end in the haloswitch quick break), and one Tmag < 6 star without a trail whose aperture run
succeeds.  Sector-2 times around the split at 1368.0, one flagged cadence, NaN pixels, one pixel below ``minflux``.
"""
import numpy as np
from scipy.special import erf

ROW0, COL0 = 200, 300
#: row, column (relative to the region), Tmag, trail half-length, trail direction (0: along the column, 1: along the row)
STARS = [
	(30.3, 25.6, 11.0, 0, 0), (31.9, 60.2, 9.5, 0, 0), (70.4, 20.7, 12.5, 0, 0),
	(8.4, 100.3, 5.5, 40, 0),      # trail into the lower row limit; its Halo stamp is clipped there
	(111.2, 60.6, 5.6, 40, 0),     # trail into the upper row limit
	(60.3, 8.2, 5.4, 40, 1),       # trail into the left column limit
	(60.7, 95.4, 5.9, 0, 0),       # bright, no trail: the aperture run succeeds
	(14.2, 106.1, 12.0, 0, 0),     # a catalogue neighbour on a mask pixel of the first bright star
]
BRIGHT_SWITCHING = (104, 105, 106)
BRIGHT_KEPT = 107
NEIGHBOUR = 108


def region(seed=3, R=120, C=130, T=24):
	"""``frames`` (dict of float32 ``(R, C, T)``), ``row0``, ``col0``, ``time``, ``quality``, ``catalog``, ``targets``."""
	rng = np.random.default_rng(seed)
	rr, cc = np.arange(R) + ROW0, np.arange(C) + COL0
	img = np.zeros((R, C))
	for (r, c, tmag, trail, along_row) in STARS:
		r, c = r + ROW0, c + COL0
		flux = 10**(-0.4 * (tmag - 20.451))
		sig = 0.6 if trail else 0.9
		pr = 0.5 * (erf((rr + 0.5 - r) / (np.sqrt(2) * sig)) - erf((rr - 0.5 - r) / (np.sqrt(2) * sig)))
		pc = 0.5 * (erf((cc + 0.5 - c) / (np.sqrt(2) * sig)) - erf((cc - 0.5 - c) / (np.sqrt(2) * sig)))
		img += flux * np.outer(pr, pc)
		if trail:
			ri, ci = int(round(r)) - ROW0, int(round(c)) - COL0
			if along_row:
				lo, hi = max(ci - trail, 0), min(ci + trail + 1, C)
				img[ri:ri + 2, lo:hi] += 0.02 * flux
			else:
				lo, hi = max(ri - trail, 0), min(ri + trail + 1, R)
				img[lo:hi, ci:ci + 2] += 0.02 * flux
	bkg = 100.0
	cube = img[:, :, None] * (1 + 1e-3 * rng.normal(size=T))[None, None, :]
	noise = np.sqrt(np.abs(cube) + bkg + 100.0)
	images = (cube + 30.0 + rng.normal(size=cube.shape) * noise).astype('float32')
	images[rng.random(images.shape) < 2e-4] = np.nan
	images[16, 108, :] = -500.0        # a pixel of the first bright star's mask below minflux
	frames = {'images': images, 'images_err': noise.astype('float32'), 'backgrounds': np.full(images.shape, bkg, dtype='float32')}
	time = 1367.75 + np.arange(T) * 1800.0 / 86400.0      # sector 2: the split at 1368.0 lies inside
	quality = np.zeros(T, dtype='int32')
	quality[5] = 32
	n = len(STARS)
	cat = {'starid': np.arange(n, dtype='int64') + 101, 'tmag': np.array([s[2] for s in STARS], dtype='float32'),
		'row': np.array([s[0] + ROW0 for s in STARS], dtype='float32'), 'column': np.array([s[1] + COL0 for s in STARS], dtype='float32')}
	targets = {'starid': cat['starid'].copy(), 'tmag': np.array([s[2] for s in STARS]), 'row': np.array([s[0] + ROW0 for s in STARS]),
		'column': np.array([s[1] + COL0 for s in STARS])}
	return frames, ROW0, COL0, time, quality, cat, targets


def halo_stamp(limits, row, column):
	"""The Halo stamp (halo_photometry.py:99-102): 22 x 22 centred on the pixel nearest to the target, clipped to the region."""
	r, c = int(np.round(row)), int(np.round(column))
	return (max(r - 11, limits[0]), min(r + 12, limits[1]), max(c - 11, limits[2]), min(c + 12, limits[3]))
