# -*- coding: utf-8 -*-
"""
``tp_bkg_mesh_kernel`` (csrc/fullframe.hip) against the oracle cell by cell, on the designed cells of tests/mesh_cells_common.py:
small and even counts, the strided sums either side of 256 valid pixels, every kind of masked pixel and the mask predicate at its
edges, the sort under ties, negative keys and ordered input, clips from one side, from both, of one to five passes and at the pass
cap, samples exactly on ``med +- 3 std``, the three branches of the SExtractor estimate, narrow cells with bright outliers (the
clipped keys carry 1e15 times the variance that is left), boxes that are no power of two and frames that are no multiple of the
box.  tests/test_mesh_cells_host.py shows without a GPU that every case takes the path its name says and that none of the oracle's
decisions in it is within rounding of its threshold -- so none is left out here.

Through ``tp_background_mesh`` as photometry_amd/prepare.py calls it: one launch per box size over the stack of mosaic frames, once
with the exclude and subtract images and once without.  ``nmasked`` equal, NaN pattern equal, ``mesh`` within 1e-9 (the bound
tests/test_gpu_fullframe.py holds this kernel to), the cases that are exact by construction equal; a second launch gives the same
bytes.
"""
import numpy as np
import pytest
import mesh_cells_common as mc

pytestmark = pytest.mark.gpu
RTOL = 1e-9
BOXES = (64, 16, 50, 1)


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.fixture(scope='module')
def mosaics():
	"""``{box: (Mosaic, {aux: (mesh, nmasked) of the oracle})}``: computed once, read by every test."""
	out = {}
	for box, cases in mc.all_cases().items():
		mo = mc.mosaic(cases, box)
		out[box] = (mo, {aux: mc.expected(mo.cases, aux) for aux in (True, False)})
	return out


def _launch(ctx, d_frames, shape, box, d_exclude=None, d_subtract=None):
	"""``(mesh float64, nmasked int32)`` host arrays ``(T, ny, nx)`` of one tp_background_mesh launch on dense frames."""
	T, R, C = shape
	ny, nx = -(-R // box), -(-C // box)
	mesh, nm = ctx.empty((T, ny, nx), 'float64'), ctx.empty((T, ny, nx), 'int32')
	mesh.fill_bytes(0x7b)
	nm.fill_bytes(0x7b)
	ctx._check(ctx.lib.tp_background_mesh(ctx.handle, d_frames.ptr, T, R, C, C, R * C, None if d_exclude is None else d_exclude.ptr, R * C,
		None if d_subtract is None else d_subtract.ptr, R * C, mc.FLUX_CUTOFF, int(box), mesh.ptr, nm.ptr))
	ctx.sync()
	return mesh.to_host(), nm.to_host()


def _compare(names, exact, got_mesh, got_nm, want_mesh, want_nm):
	"""One line per cell that differs from the oracle."""
	bad = []
	for k, name in enumerate(names):
		g, w = float(got_mesh[k]), float(want_mesh[k])
		if int(got_nm[k]) != int(want_nm[k]):
			bad.append(f'{name}: nmasked {int(got_nm[k])}, oracle {int(want_nm[k])} (mesh {g!r}, oracle {w!r})')
		elif np.isnan(g) != np.isnan(w):
			bad.append(f'{name}: mesh {g!r}, oracle {w!r}')
		elif not np.isnan(w) and (g != w if exact[k] else abs(g - w) > RTOL * abs(w)):
			bad.append(f'{name}: mesh {g!r}, oracle {w!r}' + (' (exact by construction)' if exact[k] else f' (relative {abs(g - w) / abs(w):.3g})'))
	return bad


@pytest.mark.parametrize('aux', [True, False], ids=['exclude_subtract', 'plain'])
@pytest.mark.parametrize('box', BOXES)
def test_cells_match_oracle(ctx, mosaics, box, aux):
	mo, want = mosaics[box]
	want_mesh, want_nm = want[aux]
	d_frames = ctx.array(mo.frames)
	kw = dict(d_exclude=ctx.array(mo.exclude), d_subtract=ctx.array(mo.subtract)) if aux else {}
	mesh, nm = _launch(ctx, d_frames, mo.shape, box, **kw)
	bad = _compare([c.name for c in mo.cases], [c.exact for c in mo.cases], mo.gather(mesh), mo.gather(nm), want_mesh, want_nm)
	assert not bad, f'box {box}: {len(bad)} of {len(mo.cases)} cells differ from the oracle:\n  ' + '\n  '.join(bad)
	# the same launch again: the same bytes
	mesh2, nm2 = _launch(ctx, d_frames, mo.shape, box, **kw)
	assert mesh.tobytes() == mesh2.tobytes() and nm.tobytes() == nm2.tobytes(), f'box {box}: a second launch gave other bytes'


def test_cell_does_not_depend_on_its_place(ctx, mosaics):
	"""The stack with its frames in reverse order: every cell keeps its bytes, wherever its frame lies."""
	mo, _ = mosaics[64]
	mesh, nm = _launch(ctx, ctx.array(mo.frames), mo.shape, 64)
	rmesh, rnm = _launch(ctx, ctx.array(np.ascontiguousarray(mo.frames[::-1])), mo.shape, 64)
	assert mesh.tobytes() == rmesh[::-1].tobytes() and nm.tobytes() == rnm[::-1].tobytes()
	assert mo.shape[0] >= 2 and mesh[0].tobytes() != mesh[1].tobytes()


def test_ragged_frames(ctx):
	"""Frames that are no multiple of the box: the padding counts into nmasked, cells with 2047, 2048 and 2049 masked pixels."""
	f, names = mc.ragged_frames()
	mesh, nm = _launch(ctx, ctx.array(f), f.shape, mc.RAGGED_BOX)
	bad = []
	for k, (want_mesh, want_nm) in enumerate(mc.ragged_expected(f)):
		bad += _compare([f'frame {k} {n}' for n in names], [False] * len(names), mesh[k].ravel(), nm[k].ravel(), want_mesh.ravel(), want_nm.ravel())
	assert not bad, 'cells differ from the oracle:\n  ' + '\n  '.join(bad)
	mesh2, nm2 = _launch(ctx, ctx.array(f), f.shape, mc.RAGGED_BOX)
	assert mesh.tobytes() == mesh2.tobytes() and nm.tobytes() == nm2.tobytes()
