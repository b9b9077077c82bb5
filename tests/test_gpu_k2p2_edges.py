# -*- coding: utf-8 -*-
"""
The edge cases of the K2P2 mask builder (tests/k2p2_common.py: ``EDGE_CASES``; what each one is and the ``claim`` that proves it run
on the CPU in tests/test_k2p2_edges_host.py) on the DEVICE, with the acceptance of the host test, through the launches that inline
k2p2_core.h:

* ``tp_k2p2_masks`` -- the LDS-resident kernel, and for stamps beyond its 160 KiB of work arrays (``plateau_huge``: 100 x 96,
  ``plateau_crowded_62x58``) the kernel on HBM scratch -- against the oracle;
* the mask + extraction launch ``tp_aperture_photometry_from_sumimage`` on a two-cadence cube of zeros, for the plateaus, the large
  clusters and the geometry cases: mask, status, flags, contamination and the catalogue flags bit for bit those of the stand-alone
  entry, as include/tessphot_hip.h promises.

Every input is a valid call.
"""
import copy
import numpy as np
import pytest
from k2p2_common import EDGE_CASES, edge_case, edge_accept
from test_gpu_k2p2 import run_device

pytestmark = pytest.mark.gpu

OUTPUTS = ('mask', 'status', 'flags', 'contamination', 'cat_in_mask')


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_edge_case_masks_entry(ctx, name):
	s, S, cuts, _claim = edge_case(name)
	got = run_device(ctx, s, S, cut_override=cuts)
	print(name, edge_accept(name, got))


def two_cadences_of_zeros(s):
	t = copy.copy(s)
	t.n_cad = 2
	t.images = np.zeros((s.n_targets, s.height, s.width, 2), dtype='float32')
	t.images_err, t.backgrounds = t.images.copy(), t.images.copy()
	t.quality, t.time = np.zeros(2, dtype='int32'), np.asarray(s.time[:2], dtype='float64')
	return t


@pytest.mark.parametrize("name", [n for n, (group, _f) in EDGE_CASES.items() if group in (1, 2, 4)])
def test_edge_case_fused_entry_equals_masks_entry(ctx, name):
	"""The launch that builds the mask and extracts the light curve in one (no threshold override exists there: both entries compute
	their own threshold from the same sum image) gives the stand-alone entry's outputs, bit for bit.

	What a case is at its OWN threshold is not always what its name says: the level flood (equal values under two markers) is reached
	through this launch by the clipped and quantised scenes (`plateau_quantised`: 19 of 32 targets, `plateau_faint15`: 11 of 48, counted
	with `k2p2_common.tied_floods` at the oracle's threshold), but NOT by `plateau_hand_flat` / `plateau_hand_terrace`: on a 9 x 9 stamp that
	is mostly plateau the KDE's mode is the plateau itself, only the one spike pixel lies above the threshold (no cluster), and the two hand-written label images are
	held to the device through the stand-alone entry (with the override) only.  Here those two check the no-cluster path."""
	from photometry_amd import engine, pipeline
	s, S, _cuts, _claim = edge_case(name)
	alone = run_device(ctx, s, S)
	batch = pipeline.ApertureBatch(ctx, two_cadences_of_zeros(s), cubes='host')
	work = pipeline.ApertureWork(ctx, batch)
	work.sumimage = ctx.array(np.ascontiguousarray(S, dtype='float64'))
	engine.aperture_photometry(ctx, batch, work, sumimage_given=True)
	ctx.sync()
	for key in OUTPUTS:
		a, b = getattr(work, key).to_host(), alone[key]
		if key == 'contamination':
			a, b = a.view('uint64'), b.view('uint64')      # bit for bit, NaN included
		np.testing.assert_array_equal(a, b, err_msg=key)
	# ... and where the threshold was not overridden for the oracle either, these outputs were held to it in the test above
