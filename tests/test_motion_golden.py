# -*- coding: utf-8 -*-
"""MovementKernel's host logic (apply_kernel / load_series / interpolate / jitter) against the reference's own
ImageMovementKernel (golden_motion.npz, made by tests/golden/make_golden_motion.py): bit for bit."""
import os
import numpy as np
import pytest
import conftest
from photometry_amd.motion import MovementKernel

GOLDEN = np.load(os.path.join(conftest.ROOT, 'tests', 'golden', 'golden_motion.npz'))
CASES = [(m, v) for m in ('translation', 'euclidian', 'affine') for v in ('nan0', 'nanlast', 'clean')]


@pytest.mark.parametrize('mode,variant', CASES)
def test_series_bit_for_bit(mode, variant):
	key = f'{mode}_{variant}'
	times, kernels, q, xy = GOLDEN[key + '_times'], GOLDEN[key + '_kernels'], GOLDEN[key + '_query'], GOLDEN['xy']
	mk = MovementKernel(warpmode=mode)
	mk.load_series(times, kernels)
	inter = np.array([mk.interpolate(t, xy) for t in q])
	np.testing.assert_array_equal(inter, GOLDEN[key + '_interpolate'])
	np.testing.assert_array_equal(mk.jitter(q, 1023.5, 517.25), GOLDEN[key + '_jitter'])
	app = np.array([mk.apply_kernel(xy, kernels[k]) for k in range(len(kernels))])
	np.testing.assert_array_equal(app, GOLDEN[key + '_apply'])


def test_wrong_shape_message():
	mk = MovementKernel(warpmode='translation')
	with pytest.raises(ValueError) as e:
		mk.load_series(np.arange(5.0), np.zeros((5, 3)))
	assert str(e.value) == str(GOLDEN['wrong_shape_message'])
