# -*- coding: utf-8 -*-
"""
The case table of tests/test_gpu_mesh_cells.py (tests/mesh_cells_common.py) held to the oracle without a GPU: every case takes the
path its name says -- number of clipping passes, sides clipped, branch of the SExtractor estimate, the pass cap -- and every case is
comparable: no decision of the oracle is close enough to its threshold for a rounding difference between two correct
implementations to flip it.  The conditions are tested at the actual values of every pass, with and without the exclude and
subtract images (two tables on the same frames).  No case is filtered out anywhere: a case that misses a condition fails here.
"""
import numpy as np
import pytest
import mesh_cells_common as mc
from oracle import backgrounds as ob

CASES = mc.all_cases()
ALL = [(box, case) for box, cases in CASES.items() for case in mc.mosaic(cases, box).cases]       # the fillers too
IDS = [f'{box}-{case.name}' for box, case in ALL]
BAND = 1e-6


def _walk(case, aux):
	"""The oracle's clip of the case pass by pass, and its estimate: dict of what the tests below look at."""
	img, mask = mc.keys_and_mask(case, aux)
	data = img[~mask].astype('float64')
	kept, trace = mc.clip_trace(data)
	np.testing.assert_array_equal(kept, ob.sigma_clip(data))            # the trace is the oracle's clip
	out = {'n': data.size, 'kept': kept, 'trace': trace, 'passes': sum(1 for p in trace if p['below'] + p['above']),
		'sides': ({'bottom'} if any(p['below'] for p in trace) else set()) | ({'top'} if any(p['above'] for p in trace) else set())}
	if kept.size == 0:
		out.update(branch='nan', ratio=None)
	else:
		med, mean, std = np.median(kept), np.mean(kept), np.std(kept)
		out['ratio'] = None if std == 0 else abs(mean - med) / std
		out['branch'] = 'mean' if std == 0 else ('mode' if out['ratio'] < 0.3 else 'median')
		want = ob.sextractor_background(kept)
		assert want == {'mean': mean, 'mode': 2.5*med - 1.5*mean, 'median': med}[out['branch']]
	return out


def test_table_covers_what_it_is_meant_to():
	names = [f'{box}-{case.name}' for box, case in ALL]
	assert len(set(names)) == len(names)
	b64 = {c.name: c for c in CASES[64]}
	for n in (0, 1, 2, 3, 4, 255, 256, 257, 4095, 4096):
		assert b64[f'count_{n}'].expect['n'] == n
	for kind in mc.MASK_KINDS + ('mixed',):
		assert f'none_valid_{kind}' in b64
	for tag in ('_4096', '_4089'):
		for kind in ('ascending', 'descending', 'all_equal', 'alternating', 'distinct', 'mixed_sign'):
			assert f'sort_{kind}{tag}' in b64
	assert 4089 % 16 != 0
	for name in ('clip_none', 'clip_top', 'clip_bottom', 'clip_both', 'clip_1_passes', 'clip_2_passes', 'clip_3_passes', 'clip_4_passes', 'clip_cap',
			'bound_on', 'bound_outside', 'estimator_std_zero', 'estimator_mode', 'estimator_median', 'mask_predicate'):
		assert name in b64
	assert sum(1 for c in CASES[64] if c.expect.get('narrow')) == 3 * 3 + 2
	assert {c.expect['n'] for c in CASES[16] if 'n' in c.expect} >= {255, 256}
	assert set(CASES) == {64, 16, 50, 1} and (50 & (50 - 1)) != 0


@pytest.mark.parametrize('box', sorted(CASES))
def test_mosaic_layout(box):
	"""Frames of at most 256 x 512, several cells per mesh row, at least two mesh rows, more than one frame for the 64-pixel boxes; and
	the oracle on the whole frames gives what it gives cell by cell."""
	mo = mc.mosaic(CASES[box], box)
	T, R, C = mo.shape
	assert R <= mc.MAX_ROWS and C <= mc.MAX_COLS and R % box == 0 and C % box == 0
	assert mo.mesh_shape[1] >= 2 and mo.mesh_shape[2] >= 2
	assert box != 64 or T >= 2
	assert len(set(mo.slots)) == len(mo.cases) == T * mo.mesh_shape[1] * mo.mesh_shape[2]
	for aux in (True, False):
		mesh, nm = mc.expected(mo.cases, aux)
		for t in range(T):
			mask = ob.stamp_mask(mo.frames[t], mc.FLUX_CUTOFF, mo.exclude[t].astype(bool) if aux else None)
			img = (mo.frames[t].astype('float64') - mo.subtract[t].astype('float64')).astype('float32') if aux else mo.frames[t]
			fm, fn = ob.mesh_statistics(img, mask, box=box)
			sel = [k for k, s in enumerate(mo.slots) if s[0] == t]
			np.testing.assert_array_equal(fn.ravel(), nm[sel])
			np.testing.assert_array_equal(fm.ravel(), mesh[sel])


def test_scramble_spreads_the_cell():
	"""The valid pixels of a sparse cell and the outliers of a clipped one reach every quarter of the key array (one wavefront of the
	kernel each), so the sort's strides 1024 and 2048 have work to do."""
	b64 = {c.name: c for c in CASES[64]}
	img, mask = mc.keys_and_mask(b64['count_255'])
	assert all((~mask).ravel()[q * 1024:(q + 1) * 1024].sum() > 32 for q in range(4))
	img, mask = mc.keys_and_mask(b64['clip_top'])
	assert all((img.ravel()[q * 1024:(q + 1) * 1024] > 150).sum() > 8 for q in range(4))
	# and the cases about the order of the input keep it
	v, _, _ = b64['sort_ascending_4096'].cell()
	assert np.all(np.diff(v.ravel()) > 0)
	v, _, _ = b64['sort_descending_4096'].cell()
	assert np.all(np.diff(v.ravel()) < 0)


@pytest.mark.parametrize('box,case', ALL, ids=IDS)
def test_case_takes_the_path_its_name_says(box, case):
	w = _walk(case, aux=True)
	e = case.expect
	for key in ('n', 'passes', 'sides', 'branch'):
		if key in e:
			assert w[key] == e[key], (case.name, key, w[key], e[key])
	if 'nmasked' in e:
		assert box * box - w['kept'].size == e['nmasked']
	if e.get('narrow'):
		# nothing but the outliers goes: the variance of the kept set is tiny beside what the clipped keys carried
		assert w['kept'].max() - w['kept'].min() < 0.05
	if e.get('cap'):
		# still clipping when the passes are used up: one pass fewer or more changes the count
		data = w['trace'][0]['data']
		assert [ob.sigma_clip(data, 3.0, m).size for m in (4, 5, 6)] == [3613, 3497, 3383]
		assert len(w['trace']) == 5 and all(p['below'] + p['above'] > 0 for p in w['trace'])


def test_pass_counts_from_one_to_the_cap():
	b64 = {c.name: c for c in CASES[64]}
	assert [_walk(b64[f'clip_{k}_passes'], True)['passes'] for k in (1, 2, 3, 4)] == [1, 2, 3, 4]
	# every pass of these removes one whole tier of outliers and nothing else
	for k in (1, 2, 3, 4):
		tr = _walk(b64[f'clip_{k}_passes'], True)['trace']
		assert [p['above'] for p in tr] == [40] * k + [0] and all(p['below'] == 0 for p in tr)


@pytest.mark.parametrize('aux', [True, False], ids=['aux', 'plain'])
@pytest.mark.parametrize('box,case', ALL, ids=IDS)
def test_case_is_comparable(box, case, aux):
	"""No sample within 1e-6 std of a clip bound in any pass, |mean - med| / std not within 1e-6 of 0.3 -- or the case is exact by
	construction: integer keys whose sums are exact in float64 in any order, and a power of two of them in every pass (mean and
	variance exact too) or a kept set of equal values."""
	w = _walk(case, aux)
	close = [p for p in w['trace'] if not p['margin'] >= BAND]
	if close:
		assert case.exact, (case.name, [p['margin'] for p in w['trace']])
	if w['ratio'] is not None:
		assert abs(w['ratio'] - 0.3) > BAND, (case.name, w['ratio'])
	if case.exact and w['n'] > 1:
		data = w['trace'][0]['data']
		assert np.all(data == np.round(data)) and np.sum(np.abs(data)) < 2.0**53 and np.sum(data * data) < 2.0**53
		pow2 = all((p['m'] & (p['m'] - 1)) == 0 for p in w['trace'])
		assert pow2 or np.all(w['kept'] == w['kept'][0]), case.name
		assert not close or pow2


def test_bound_cells():
	"""94 and 106 ON med +- 3 std are kept; one float32 step further out they go."""
	b64 = {c.name: c for c in CASES[64]}
	on, out = _walk(b64['bound_on'], True), _walk(b64['bound_outside'], True)
	p = on['trace'][0]
	assert (p['med'], p['std'], p['margin']) == (100.0, 2.0, 0.0) and on['kept'].size == 4096
	assert np.sum(on['kept'] == 94) == 8 and np.sum(on['kept'] == 106) == 8
	assert out['kept'].size == 4080 and out['kept'].min() == 98 and out['kept'].max() == 102


def test_mask_predicate_cell():
	"""Every special value on its side of the mask, and one pixel more or less moves the estimate by far more than the tolerance."""
	case = {c.name: c for c in CASES[64]}['mask_predicate']
	img, mask = mc.keys_and_mask(case)
	tiny = np.nextafter(np.float32(0), np.float32(1))
	v = img[~mask]
	assert v.size == 8 and np.sum(v == 0) == 2 and np.sum(np.signbit(v)) == 1 and np.sum(v == tiny) == 1 and np.sum(v == np.float32(8e4)) == 1
	gone = img[mask]
	for x in (np.nextafter(np.float32(8e4), np.float32(np.inf)), np.float32(-1e-30), -tiny):
		assert np.sum(gone == x) == 1
		# kept by mistake: another count, another estimate
		m2, n2 = ob.mesh_statistics(img, mask & (img != x))
		m1, n1 = ob.mesh_statistics(img, mask)
		assert n2[0, 0] == n1[0, 0] - 1 and abs(m2[0, 0] / m1[0, 0] - 1) > 1e-3
	for x in (np.float32(8e4), tiny):
		m2, n2 = ob.mesh_statistics(img, mask | (img == x))
		assert n2[0, 0] == n1[0, 0] + 1 and abs(m2[0, 0] / m1[0, 0] - 1) > 1e-3


def test_ragged_frames():
	f, names = mc.ragged_frames()
	T, R, C = f.shape
	assert R % mc.RAGGED_BOX and C % mc.RAGGED_BOX and len(names) == 8
	for k, (mesh, nm) in enumerate(mc.ragged_expected(f)):
		assert mesh.shape == (2, 4) and np.all(np.isfinite(mesh))
		full, half = 64 * 64, 64 * 64 // 2
		np.testing.assert_array_equal(nm, [[0, 0, 0, full - 64 * 40], [half - 1, half, half + 1, full - 33 * 40]])
		# nothing is clipped in these cells: the counts are the padding and the NaNs alone, and the cells are comparable
		for j in range(2):
			for i in range(4):
				cell = f[k, j * 64:(j + 1) * 64, i * 64:(i + 1) * 64]
				kept, trace = mc.clip_trace(cell[np.isfinite(cell)])
				assert len(trace) == 1 and trace[0]['margin'] > BAND
				assert abs(abs(np.mean(kept) - np.median(kept)) / np.std(kept) - 0.3) > BAND
