# -*- coding: utf-8 -*-
"""
The edge cases of the K2P2 mask builder (tests/k2p2_common.py: ``EDGE_CASES``) through the HOST build of
photometry_amd/csrc/k2p2_core.h (tests/hostsim), against the oracle.  The same cases run on the device in
tests/test_gpu_k2p2_edges.py; here each case's ``claim`` is asserted as well: from the oracle's side alone, the case is the case its
name says (equal values under two markers, an empty KDE sample, a target that wraps to the last row, ...).

The cases exist for the BRANCHES of the builder that ordinary scenes leave untaken.  To measure them (lines and branches of
k2p2_core.h over this module and tests/test_k2p2_hostsim.py together), from the repository's root:

    K2P2_HOSTSIM_COVERAGE=1 python -m pytest -q tests/test_k2p2_hostsim.py tests/test_k2p2_edges_host.py && (cd tests/hostsim/build && gcov -b k2p2_hostsim_cov-k2p2_hostsim | grep -A4 "k2p2_core.h'")

(``K2P2_HOSTSIM_COVERAGE=1``: ``k2p2_common.build_hostsim`` compiles the host library with ``-O0 --coverage``; the annotated source, every
untaken branch marked, is then tests/hostsim/build/k2p2_core.h.gcov.)

With both modules: 100 % of the lines, 95.45 % of 1 210 branches taken at least once.  The 55 that are not, by construct:

* the host shim always passes ``t.diag`` and ``t.cat_in_mask`` (six ``if (t.diag)`` / ``if (t.cat_in_mask)``); ``prm.extend_overflow`` and
  ``prm.ws_thres`` are the plugin's fixed settings; the exception edges gcov gives the calls of ``func`` / ``neg_kde`` / ``sp_brent`` /
  ``sp_bracket`` / ``threshold`` in a host build;
* scipy's safety nets in ``sp_bracket`` / ``sp_brent`` / ``powell_mode``: the ``verysmall`` denominator, the iteration and call caps, ``fw > fb``
  after a parabolic step, a zero direction (``direc1 != 0.0`` false), one operand of the NaN exit, ``t < 0`` false;
* ``tp_exp`` overflow (its arguments are <= 0); a NaN standard deviation with a positive IQR (a sample of one has IQR 0); ``lxi`` beyond
  1e9; the grid's bin bounds ``m < M``; a NaN density in the upper half of the grid only; the argmax on the last grid point;
* windows and reflections one pixel wide (``win_make`` empty, ``v.w > 1`` false, ``reflect_idx(n == 1)``): a DBSCAN core needs four pixels in a
  3 x 3 neighbourhood, so a cluster spans two rows and two columns at least, and a stamp one pixel across has no cluster;
* ``saturated_one``: a mask of NaN pixels only, ``imax < 0``, ``imax`` off the column or off ``idx`` (the column's maximum is a pixel above the threshold);
* the peak threshold below zero (``max(min, 0 * max)`` is never negative); ``bi < 0`` (no peak with a catalogue: raised before); a NaN
  distance against a finite one, either way (a star's distances are all NaN or none); ``p < bi`` false among equal intensities (the host
  build lists peaks in raster order); NaN in the blurred image of the saturated de-duplication;
* seeds of the flood's summary words beyond word 31 (a marker of rank >= 1 024: markers are among a cluster's brightest pixels);
* ``room`` false (5 clusters per 2 pixels), ``!err`` in the two loop conditions (an error leaves by ``break``).
"""
import pytest
from k2p2_common import EDGE_CASES, edge_case, edge_reference, edge_accept, build_hostsim, run_hostsim


@pytest.fixture(scope='module')
def hostsim():
	return build_hostsim()


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_edge_case_hostsim(hostsim, name):
	s, S, cuts, claim = edge_case(name)
	ref = edge_reference(name)
	claim(ref, s, S, cuts)
	got = run_hostsim(hostsim, s, S, cut_override=cuts)
	print(name, edge_accept(name, got))
