#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Generator of ``golden_motion.npz``: the host logic of the reference's ``ImageMovementKernel`` (photometry/image_motion.py) --
``apply_kernel``, ``load_series``, ``interpolate`` and ``jitter`` (:113-421) -- run on seeded kernel series through
``_refstub`` (cv2, skimage and astropy stubbed: these methods do not touch them outside ``'wcs'``).

The series hold NaN kernels (one of them at index 0, whose NaN is the interpolator's lower fill value), the query times fall
inside, on and outside the range, for the three numeric warp modes.  ``tests/test_motion_golden.py`` holds
``photometry_amd.motion.MovementKernel`` to these values bit for bit.

Run on a machine with the reference checkout (``python tests/golden/make_golden_motion.py [--out DIR]``, by default into this
directory); the result is committed, and ``tests/test_golden_regenerates.py`` holds a fresh run to it.
"""

import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refstub # noqa: E402

sys.meta_path.insert(0, _refstub._StubFinder())
_refstub.import_reference()
from photometry.image_motion import ImageMovementKernel # noqa: E402

MODES = ('translation', 'euclidian', 'affine')


def series(mode, rng, T=40):
	n = ImageMovementKernel.N_PARAMS[mode]
	times = 1500.0 + np.cumsum(rng.uniform(0.015, 0.025, T))
	if mode == 'affine':
		kernels = np.tile([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], (T, 1)) + rng.normal(0, 1e-4, (T, 6))
		kernels[:, [2, 5]] += rng.normal(0, 0.3, (T, 2))
	else:
		kernels = rng.normal(0, 0.3, (T, n))
		if mode == 'euclidian':
			kernels[:, 2] = rng.normal(0, 1e-4, T)
	return times, kernels


def main(out_dir=HERE):
	rng = np.random.default_rng(20261015)
	out = {}
	xy = np.array([[10.5, 20.25], [1000.0, 1500.0], [2047.0, 0.0], [431.7, 1777.3]])
	for mode in MODES:
		for variant, nan_rows in (('nan0', [0, 7, 8, 23]), ('nanlast', [5, 39]), ('clean', [])):
			times, kernels = series(mode, rng)
			kernels[nan_rows, :] = np.nan
			imk = ImageMovementKernel(warpmode=mode)
			imk.load_series(times, kernels)
			q = np.concatenate([[times[0] - 0.1, times[0], times[-1], times[-1] + 0.3], times[3:10], rng.uniform(times[0], times[-1], 25)])
			inter = np.array([imk.interpolate(t, xy) for t in q])
			jit = imk.jitter(q, 1023.5, 517.25)
			app = np.array([imk.apply_kernel(xy, kernels[k]) for k in range(len(kernels))])
			key = f'{mode}_{variant}'
			out[key + '_times'] = times
			out[key + '_kernels'] = kernels
			out[key + '_query'] = q
			out[key + '_interpolate'] = inter
			out[key + '_jitter'] = jit
			out[key + '_apply'] = app
	out['xy'] = xy
	# load_series' shape check: the message is part of the behaviour
	imk = ImageMovementKernel(warpmode='translation')
	try:
		imk.load_series(np.arange(5.0), np.zeros((5, 3)))
	except ValueError as e:
		out['wrong_shape_message'] = np.array(str(e))
	np.savez_compressed(os.path.join(out_dir, 'golden_motion.npz'), **out)


if __name__ == '__main__':
	import argparse
	parser = argparse.ArgumentParser(description="Write golden_motion.npz by executing the reference.")
	parser.add_argument('--out', default=HERE, metavar='DIR', help="directory the fixture is written to (default: this directory)")
	args = parser.parse_args()
	os.makedirs(args.out, exist_ok=True)
	main(os.path.abspath(args.out))
