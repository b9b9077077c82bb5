# -*- coding: utf-8 -*-
"""
The oracle of the light-curve diagnostics (oracle/diagnostics.py) on every case of tests/diagnostics_common.py, without a GPU:
it raises nothing, and it returns the flags that the construction of the case implies, written out here as known answers
(1 all fluxes NaN, 2 all errors NaN, 4 invalid time vector, 8 no detrending).  tests/test_gpu_diagnostics_edges.py holds the
kernel to these rows, so a case that silently stopped being what its name says would be caught here.

Where the reference checkout is present, ``oracle.utilities.rms_timescale`` is compared bit for bit with the reference's own
``utilities.rms_timescale`` on every time-axis case with a valid time vector (one fresh interpreter for all of them: importing
the reference installs import hooks).
"""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import diagnostics_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
from _refstub import REFERENCE_PATH # noqa: E402  (the probe of missing packages it runs on import changes nothing)


def rows(case):
	return dc.oracle_rows(*case)


@pytest.mark.parametrize('T', [255, 256, 257])
def test_selection(T):
	case = dc.selection_case(T)
	time, quality, flux, ferr, cen, kwargs = case
	out = rows(case)
	assert [r['flags'] for r in out] == [0] * len(dc.SELECTION_TARGETS)
	t = {k: i for i, k in enumerate(dc.SELECTION_TARGETS)}
	good = dc.good_of(quality, 0, kwargs)
	# the cases are what their names say
	assert out[t['negative flux']]['mean_flux'] < 0 and np.all(flux[t['negative flux']] < 0)
	assert out[t['ties at both middle ranks']]['mean_flux'] == 101.0
	r = out[t['middle ranks differ above duplicates']]
	assert r['mean_flux'] == 102.0 and r['pos_centroid_col'] == 102.0 and r['pos_centroid_row'] == -102.0
	i = t['middle ranks differ above duplicates']
	assert np.sum(flux[i][good] == 101.0) > 10 and np.sum(~np.isnan(flux[i][good])) % 2 == 0
	assert out[t['two values']]['mean_flux'] == 6.0
	r = out[t['all equal']]
	assert (r['mean_flux'], r['variance'], r['rms_hour'], r['ptp'], r['variability']) == (7.5, 0, 0, 0, 0)
	r = out[t['+inf and -inf']]
	assert np.isfinite(r['mean_flux']) and np.isfinite(r['ptp']) and np.isfinite(r['rms_hour']) and np.isnan(r['variance'])
	assert np.isfinite(r['pos_centroid_col']) and np.isfinite(r['pos_centroid_row'])
	r = out[t['signed zeros']]
	assert r['pos_centroid_col'] == 0 and r['pos_centroid_row'] == 0
	i = t['600 decades and subnormals']
	c = np.abs(cen[i][good])
	assert c.min() < 2.3e-308 and c.min() > 0 and c.max() > 1e295 and np.sum(c < 2.2250738585072014e-308) >= 10
	assert np.any(cen[i][good][:, 1] < 0) and np.any(cen[i][good][:, 1] > 0)


@pytest.mark.parametrize('bitmask,expected', [
	(dc.DEFAULT_BITMASK, [8, 12, 8, 8, 0, 0, 8, 8]), # 0, 1, 2, 3, 4, 5, 3 good cadences and 4 that are all NaN
	(16, [0, 0, 8, 8, 12, 8, 0, 8])])                # 5, 4, 3, 2, 1, 0, 4, 3
def test_few_good_cadences(bitmask, expected):
	"""No good cadence: 8 and NaNs.  One: the time span is zero (4) and the fit has one point (8; numpy's polyfit ends in a
	LinAlgError there, which the reference does not catch).  Two and three: the cubic is rank deficient (8).  Four and more: none."""
	case = dc.few_good_case(bitmask)
	time, quality, flux, ferr, cen, kwargs = case
	assert quality.ndim == 2 and kwargs == {'bitmask': bitmask}
	counts = [int(np.sum(dc.good_of(quality, i, kwargs))) for i in range(len(flux))]
	assert counts == dc.few_good_counts(bitmask)
	assert sorted(set(counts)) == [0, 1, 2, 3, 4, 5]
	out = rows(case)
	assert [r['flags'] for r in out] == expected
	for n, r in zip(counts, out):
		if n == 0:
			assert all(np.isnan(r[k]) for k in dc.EXACT[:4] + ('variance', 'rms_hour', 'variability'))
		if n == 1:
			assert r['variability'] == 0 and np.isnan(r['variance']) and np.isnan(r['rms_hour']) and np.isnan(r['ptp'])
	if bitmask == dc.DEFAULT_BITMASK: # the good cadences are all NaN, the flagged ones are not: no ALLNAN flag, every series value NaN
		i = dc.FEW_GOOD_NAN_TARGET
		assert np.all(np.isnan(flux[i][dc.good_of(quality, i, kwargs)])) and not np.all(np.isnan(flux[i]))
		assert np.isnan(out[i]['mean_flux']) and np.isnan(out[i]['variability']) and not np.isnan(out[i]['pos_centroid_col'])
	fitted = [dc.fitted_cadences(time, quality, flux, ferr, i, kwargs) for i in range(len(flux))]
	assert all(f in (0, n) for f, n in zip(fitted, counts))


TIME_FLAGS = {'inf_time': 4, 'three_stamps': 8}


@pytest.mark.parametrize('name', dc.TIME_CASES)
def test_time_axis(name):
	case = dc.time_case(name)
	time, quality, flux, ferr, cen, kwargs = case
	assert len(time) <= 300 and flux.shape[0] <= 32
	out = rows(case)
	assert [r['flags'] for r in out] == [TIME_FLAGS.get(name, 0)] * len(flux)
	for r in out:
		assert np.isnan(r['rms_hour']) == (name == 'inf_time')
		assert np.isfinite(r['mean_flux']) and np.isfinite(r['ptp']) and np.isfinite(r['variance'])
	good = dc.good_of(quality, 0, kwargs)
	t = time[good]
	ts = kwargs.get('timescale', dc.HOUR)
	if name in ('grid_dyadic', 'grid_hour', 'on_edges', 'below_edges'):
		edges = dc.arange_edges(t.min(), t.max(), ts)
		assert np.array_equal(edges, np.arange(t.min(), t.max(), ts))
		on = np.isin(t, edges)
		guess = np.floor((t - t.min()) / ((t.min() + ts) - t.min())).astype(int)
		right = np.minimum(np.searchsorted(edges, t, side='right') - 1, len(edges) - 1)
		if name == 'grid_dyadic':
			assert np.sum(on) >= len(t) // 2 - 1
		if name in ('on_edges', 'below_edges'): # the first guess of the bin is wrong for many samples: too low in one case, too high in the other
			assert np.sum(on) >= len(t) // 2 - 1
			assert np.sum(guess < right if name == 'on_edges' else guess > right) >= 20
	if name == 'duplicate':
		assert np.sum(np.diff(t) == 0) == 3
	if name.endswith('permuted'):
		assert np.any(np.diff(t) < 0)
	elif name not in ('nan_time', 'inf_time'):
		assert np.all(np.diff(t) >= 0)
	if name.startswith('bins'):
		assert dc.n_bins(time, quality, kwargs) == (256 if name == 'bins256' else 257) and len(time) <= 256
	else:
		assert name == 'inf_time' or dc.n_bins(time, quality, kwargs) <= 256


def test_permutation_keeps_the_medians():
	a, b = rows(dc.time_case('grid_hour')), rows(dc.time_case('permuted'))
	for x, y in zip(a, b):
		assert x['mean_flux'] == y['mean_flux'] and x['pos_centroid_col'] == y['pos_centroid_col'] and x['ptp'] != y['ptp']


def test_degenerate_flux():
	"""A median of exactly 0 with non-zero samples: ``rel`` is +-inf or NaN, no sample is finite, ``binned_statistic`` raises its
	ValueError on the empty selection (4) and the fit has no point (8).  All-zero flux: ``rel`` is all NaN, which rms_timescale
	answers with NaN before it looks at the time (8 only)."""
	case = dc.degenerate_case()
	out = rows(case)
	assert [r['flags'] for r in out] == [0, 12, 8, 0, 0]
	assert out[0]['mean_flux'] < 0 and np.isfinite(out[0]['variability'])
	assert out[1]['mean_flux'] == 0 and np.any(case[2][1] != 0) and np.isnan(out[1]['rms_hour']) and out[1]['ptp'] == np.inf
	assert out[2]['mean_flux'] == 0 and np.isnan(out[2]['ptp'])
	assert np.isfinite(out[3]['rms_hour']) and np.isnan(out[3]['variance'])


def test_lds_boundary_sizes():
	"""The restated host formula: 24 bytes per cadence beside 4 136 bytes of fixed scratch under 160 KiB."""
	n = dc.lds_boundary()
	assert n == dc.lds_boundary(9, 13) and 6000 < n < 7000
	assert 4136 + ((24 * n + 15) & ~15) <= 160 * 1024 < 4136 + ((24 * (n + 1) + 15) & ~15)


def test_timescale_keyword():
	"""``timescale`` reaches rms_timescale; the default is the reference's hour."""
	from oracle import diagnostics as odiag
	from oracle.utilities import rms_timescale
	time, quality, flux, ferr, cen, kwargs = dc.time_case('grid_hour')
	good = dc.good_of(quality, 0, kwargs)
	rel = flux[0][good] / np.nanmedian(flux[0][good]) - 1
	assert odiag.diagnostics(time, quality, flux[0], ferr[0], cen[0])['rms_hour'] == rms_timescale(time[good], rel, timescale=dc.HOUR)
	r = odiag.diagnostics(time, quality, flux[0], ferr[0], cen[0], timescale=0.5)['rms_hour']
	assert r == rms_timescale(time[good], rel, timescale=0.5) != rms_timescale(time[good], rel)
	assert odiag.FLAG_TOO_MANY_BINS == 16


#--------------------------------------------------------------------------------------------------
_REFERENCE_RMS = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import _refstub
sys.meta_path.insert(0, _refstub._StubFinder())
photometry = _refstub.import_reference()
from photometry.utilities import rms_timescale
import diagnostics_common as dc
out = {}
for name in dc.TIME_CASES:
	if name == 'inf_time':
		continue
	time, quality, flux, ferr, cen, kwargs = dc.time_case(name)
	good = dc.good_of(quality, 0, kwargs)
	out[name] = []
	for i in range(len(flux)):
		rel = flux[i][good] / np.nanmedian(flux[i][good]) - 1
		out[name].append(float(rms_timescale(time[good], rel, timescale=kwargs.get('timescale', dc.HOUR))).hex())
print('RESULT ' + json.dumps(out))
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE_PATH, 'photometry')),
	reason=f"the reference checkout ({REFERENCE_PATH}) is not on this machine: its rms_timescale cannot be called here")
def test_rms_timescale_equals_the_reference():
	from oracle.utilities import rms_timescale
	r = subprocess.run([sys.executable, '-c', _REFERENCE_RMS, GOLDEN, os.path.join(ROOT, 'tests')], cwd=ROOT, capture_output=True, text=True, timeout=120)
	assert r.returncode == 0, r.stderr[-3000:]
	ref = json.loads([line for line in r.stdout.splitlines() if line.startswith('RESULT ')][-1][7:])
	assert sorted(ref) == sorted(n for n in dc.TIME_CASES if n != 'inf_time')
	for name, values in ref.items():
		time, quality, flux, ferr, cen, kwargs = dc.time_case(name)
		good = dc.good_of(quality, 0, kwargs)
		for i, h in enumerate(values):
			rel = flux[i][good] / np.nanmedian(flux[i][good]) - 1
			mine = rms_timescale(time[good], rel, timescale=kwargs.get('timescale', dc.HOUR))
			assert float(mine).hex() == h and np.isfinite(mine), (name, i, mine, float.fromhex(h))
