# -*- coding: utf-8 -*-
"""
What the CPU test of the radial background's rules (test_radial_rules_host.py) and the GPU test of the ring kernel on hand-made
rings (test_gpu_fullframe.py) share: the oracle's ring mode together with the margin by which its argmax is decided, and the
comparison of a ring mode with it.

A ring mode is the argmax over a 2048-point KDE grid, so a comparison "on the same grid point" (``|diff| < 2e-5``: a grid step of
these rings is 1e-5 .. 5e-4) means something only where the oracle's own argmax is not decided by rounding.  ``separation`` is
``(d1 - d2) / d1`` of the oracle's largest and second-largest density value.  Measured on ``2.0 + normal(0, 2e-3, n)``, seeds 3 and 4,
``n`` = 3 .. 4097: the densities of the serial host composition (glibc ``exp`` / ``sin`` / ``cos``, radix-2 transform) and of the oracle
(pocketfft), each divided by its maximum, differ by 7e-16 at most, and the smallest separation is 2e-8; ``SEPARATION`` = 1e-9 leaves
six orders of magnitude above that rounding and is asserted on the oracle alone for every ring of three or more samples.

Two samples are the one case no seed helps: the bandwidth is 0.34 of their distance, the density has two mirror-image peaks, and
the oracle's own pick between them is rounding (measured: separation 0 .. 2e-16; over 40 seeds the host composition took the
oracle's peak 29 times).  There the comparison is with the tied pair: the oracle's two largest density values must be the mirror
pair (asserted), and the mode must be one of these two grid points.
"""
import numpy as np
from oracle import kde as okde

BW_CONSTANT = okde.normal_reference_constant()
SEPARATION = 1e-9
SAME_GRID_POINT = 2e-5          # the criterion of test_fit_background_tess_matches_oracle


def oracle_ring_mode(x):
	"""``oracle.backgrounds.reduce_mode(x, binning='fixed')`` statement for statement, with what decided it: returns ``(mode,
	separation, tied)`` -- ``separation`` None where no argmax is taken (NaN mode, or zero bandwidth: the median), ``tied`` the grid
	values of the two largest density values."""
	if len(x) == 0:
		return np.nan, None, None
	x = np.asarray(x, dtype='float64')
	kde = okde.KDE(x)
	try:
		with np.errstate(all='ignore'):
			kde.fit(gridsize=2000, binning='fixed')
	except RuntimeError as err:
		if str(err).startswith('Selected KDE bandwidth is 0.'):
			return np.median(x), None, None
		raise
	mode = kde.support[np.argmax(kde.density)]
	if np.isnan(mode):
		return mode, None, None
	top = np.argsort(kde.density, kind='stable')[::-1][:2]
	d1, d2 = kde.density[top]
	return mode, (d1 - d2) / d1, (kde.support[top], top)


def assert_same_mode(got, x, label=''):
	"""``got`` against the oracle's mode of the samples ``x``; returns which rule applied ('nan', 'median', 'tie', 'argmax')."""
	mode, separation, tied = oracle_ring_mode(x)
	if np.isnan(mode):
		assert np.isnan(got), (label, got)
		return 'nan'
	assert not np.isnan(got), (label, mode)
	if separation is None:
		assert got == mode, (label, got, mode)                  # zero bandwidth: the median, exact
		return 'median'
	if len(x) == 2:
		support, top = tied
		assert top[0] + top[1] == 2047 and separation < 1e-12, (label, top, separation)      # the mirror pair, tied
		assert np.min(np.abs(got - support)) < SAME_GRID_POINT, (label, got, support)
		return 'tie'
	assert separation > SEPARATION, (label, len(x), separation)                              # on the oracle alone
	assert abs(got - mode) < SAME_GRID_POINT, (label, len(x), got, mode)
	return 'argmax'
