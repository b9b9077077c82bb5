# -*- coding: utf-8 -*-
"""
``bench.py --dump-outputs``: benchlib.dump on the arrays ``ShardedRun.collect`` returns (output blocks of comm.packed_block_layout
filled with seeded bytes, NaN and infinities among the floats, reassembled as on rank 0): every file in float32 / float64 and
finite, every array rebuilt exactly from its files, the same fixed sample of targets in every file when the set exceeds the
budget, and the budget held.
"""
import os
import numpy as np
import pytest
from benchlib import dump
from photometry_amd import comm


def _outputs(sizes, T, H, psf):
	layout, nbytes = comm.packed_block_layout(max(sizes), T, H, H, psf=psf)
	rng = np.random.default_rng(7)
	blocks = []
	for _ in sizes:
		blk = np.zeros(nbytes, dtype='uint8')
		for name, (off, shape, dt) in layout.items():
			n = int(np.prod(shape))
			if np.dtype(dt).kind == 'f':
				v = rng.normal(size=n).astype(dt)
				v[rng.random(n) < 0.05] = np.nan
				v[:2] = (np.inf, -np.inf)
			else:
				v = rng.integers(0, 2 if name == 'mask' else 1 << 20, size=n).astype(dt)
			blk[off:off + v.nbytes] = v.view('uint8')
		blocks.append(blk)
	return comm.assemble_blocks(blocks, layout, sizes)


def _read(d):
	got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
	for name, a in got.items():
		assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
	return got


def _rebuilt(got, name):
	"""The array as the caller had it: the values, with the non-finite entries put back from their codes."""
	code = got.get(name + dump.NONFINITE_SUFFIX)
	if code is None:
		return got[name]
	assert code.shape == got[name].shape and code.dtype == np.float32 and np.all(got[name][code != 0] == 0)
	return np.where(code == 0, got[name], np.choose(code.astype(int), [0.0, np.nan, np.inf, -np.inf]).astype(got[name].dtype))


def test_everything_written_when_it_fits(tmp_path):
	out = _outputs([5, 4], 30, 7, psf=True)
	idx = dump.dump_outputs(out, str(tmp_path), 9)
	got = _read(str(tmp_path))
	floating = {name for name, a in out.items() if a.dtype.kind == 'f'}
	assert floating == {'lc', 'contamination', 'psf_flux', 'psf_contamination'}
	assert set(got) == set(out) | {'target_index'} | {name + dump.NONFINITE_SUFFIX for name in floating}
	np.testing.assert_array_equal(idx, np.arange(9))
	np.testing.assert_array_equal(got['target_index'], np.arange(9))
	for name, a in out.items():
		if name in floating:
			assert got[name].dtype == a.dtype, name
		np.testing.assert_array_equal(_rebuilt(got, name), a)        # exact: integers widened, floats and their NaN / inf as they are
	assert (got['lc_nonfinite'] == 1).any() and (got['lc_nonfinite'] == 2).any() and (got['lc_nonfinite'] == 3).any()
	assert got['mask'].dtype == np.float32 and got['status'].dtype == np.float64


def test_a_fixed_sample_within_the_budget(tmp_path):
	out = _outputs([40, 40, 37], 50, 5, psf=False)
	budget = 200000
	idx = dump.dump_outputs(out, str(tmp_path / 'a'), 117, max_bytes=budget)
	again = dump.dump_outputs(out, str(tmp_path / 'b'), 117, max_bytes=budget)
	assert 0 < len(idx) < 117 and np.all(np.diff(idx) > 0)
	np.testing.assert_array_equal(idx, again)                          # the same targets from run to run
	assert sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')) <= budget
	got = _read(str(tmp_path / 'a'))
	np.testing.assert_array_equal(got['target_index'], idx)
	np.testing.assert_array_equal(_rebuilt(got, 'lc'), out['lc'][:, idx])
	for name in ('contamination', 'status', 'flags', 'mask'):
		np.testing.assert_array_equal(_rebuilt(got, name), out[name][idx])


def test_refuses_what_cannot_be_written(tmp_path):
	out = _outputs([3], 20, 5, psf=False)
	with pytest.raises(ValueError):
		dump.dump_outputs(out, str(tmp_path), 4)                       # no target axis of that length
	with pytest.raises(ValueError):
		dump.dump_outputs(out, str(tmp_path), 3, max_bytes=33000)     # not even one target fits (eight files, up to 4 KB of header each)
