# -*- coding: utf-8 -*-
"""
``tpf.load_tpf_groups``: target pixel files unpacked straight into cubes of many targets, one set of cubes per ``(H, W, T)``.  Seven
files of random bit patterns (tests/tpf_common.py: NaN payloads, signalling NaNs, denormals): four of 11 x 11 x 70, the first of
them with two non-finite ``TIME`` rows in the middle, two of 7 x 9 x 70 and one of 1 x 1 x 33.  Every slot is held bit for bit, pads
included, to the cube ``tpf.load_tpfs`` makes of that file alone; the odd file, first in the list, leaves the hole that the last
regular file has to fill.
"""
import numpy as np
import pytest
import ffi_common as fc
import tpf_common as tc
from alloc_common import count_allocations
from photometry_amd import ffi, tpf

pytestmark = pytest.mark.gpu

#: (H, W, rows, rows without a finite TIME), in the order the files are loaded
FILES = ((11, 11, 70, (30, 31)), (7, 9, 70, ()), (11, 11, 70, ()), (1, 1, 33, ()), (11, 11, 70, ()), (7, 9, 70, ()), (11, 11, 70, ()))
NAMES = ('images', 'images_err', 'backgrounds')


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


@pytest.fixture(scope='module')
def seven(tmp_path_factory):
	root = tmp_path_factory.mktemp('tpfgroups')
	rng = np.random.default_rng(404)
	made = [tc.make_tpf(rng, H, W, n, bad_times=bad, crval1p=100 + 20 * k, crval2p=50 + 7 * k, primary=dict(TICID=1000 + k)) for k, (H, W, n, bad) in enumerate(FILES)]
	files = [fc.write(root / ('tess2019199201929-s0014-%016d-0150-s_tp.fits' % (1000 + k)), made[k][0]) for k in range(len(FILES))]
	return {'files': files, 'made': made}


@pytest.fixture(scope='module')
def reference(ctx, seven):
	"""Every file through ``load_tpfs``, once: the full cubes (pads included) on the host."""
	loaded = tpf.load_tpfs(ctx, seven['files'])
	ref = [{name: ld.cubes[name].data.to_host()[0] for name in NAMES} for ld in loaded]
	pitch = [ld.cubes['images'].t_pitch for ld in loaded]
	for ld in loaded:
		ld.free()
	return loaded, ref, pitch


@pytest.fixture(scope='module')
def grouped(ctx, seven):
	groups, index = tpf.load_tpf_groups(ctx, seven['files'])
	yield groups, index
	for g in groups:
		g.free()


def test_groups_and_input_order(seven, grouped):
	groups, index = grouped
	assert [g.shape for g in groups] == [(11, 11, 70), (11, 11, 68), (7, 9, 70), (1, 1, 33)]
	# the odd file sits in a group of its own; the last regular 11 x 11 file filled its slot: slots 0..2 of one cube
	assert index == [(1, 0), (2, 0), (0, 1), (3, 0), (0, 2), (2, 1), (0, 0)]
	assert [len(g) for g in groups] == [3, 1, 2, 1]
	for i, (g, s) in enumerate(index):
		assert groups[g].loaded[s].path == seven['files'][i] and groups[g].loaded[s].header['TICID'] == 1000 + i
	big = groups[0].cubes['images']
	assert (big.n_targets, big.n_cad, big.height, big.width, big.t_pitch) == (3, 70, 11, 11, 96)
	one = 11 * 11 * 96 * 4
	assert [groups[0].loaded[s].cubes['images'].ptr for s in range(3)] == [big.ptr + s * one for s in range(3)]


def test_every_slot_is_the_cube_load_tpfs_makes(seven, reference, grouped):
	groups, index = grouped
	loaded, ref, pitch = reference
	for i, (g, s) in enumerate(index):
		grp = groups[g]
		H, W, T = grp.shape
		for name in NAMES:
			cube = grp.cubes[name]
			assert (cube.n_targets, cube.n_cad, cube.height, cube.width) == (len(grp), T, H, W)
			assert cube.t_pitch == pitch[i]                                   # (the shapes of this test: the pitch from NAXIS2 is the pitch from T)
			got = cube.data.to_host()[s]
			assert got.shape == ref[i][name].shape and np.array_equal(got.view('uint32'), ref[i][name].view('uint32')), (i, name)
			assert np.all(got[:, :, T:].view('uint32') == 0)
			view = grp.loaded[s].cubes[name]
			assert (view.n_targets, view.n_cad, view.t_pitch) == (1, T, cube.t_pitch)
			assert np.array_equal(view.data.to_host()[0].view('uint32'), ref[i][name].view('uint32'))
		blob, rec, ap, info = seven['made'][i]
		good = np.isfinite(rec['TIME'])
		assert T == int(good.sum())
		assert np.array_equal(grp.cubes['images'].to_host()[s].view('uint32'), tc.host_cube(rec, 'FLUX', good))   # and numpy's own reading


def test_group_vectors_and_apertures(seven, reference, grouped):
	groups, index = grouped
	loaded, ref, pitch = reference
	for i, (g, s) in enumerate(index):
		grp, want = groups[g], loaded[i]
		n, (H, W, T) = len(grp), grp.shape
		assert grp.time.shape == (n, T) and grp.time.dtype == np.float64 and grp.quality.shape == (n, T) and grp.quality.dtype == np.int32
		assert grp.aperture.shape == (n, H, W) and grp.aperture.dtype == np.int32
		assert np.array_equal(grp.time[s].view('uint64'), want.time.view('uint64')) and np.array_equal(grp.quality[s], want.quality)
		assert np.array_equal(grp.aperture[s], want.aperture & ~(2 | 8)) and not np.any(grp.aperture[s] & (2 | 8))
		mine = grp.loaded[s]
		for key in ('timecorr', 'cadenceno', 'pos_corr', 'aperture'):
			a, b = getattr(mine, key), getattr(want, key)
			assert a.dtype == b.dtype and np.array_equal(a.view('uint8'), b.view('uint8')), key
		for key in ('max_stamp', 'wcs_cards', 'sector', 'camera', 'ccd', 'data_rel', 'cadence', 'readnoise', 'gain', 'num_frm', 'n_readout', 'rows_dropped',
			'time_offset_corrected', 'header'):
			assert getattr(mine, key) == getattr(want, key), key
	assert groups[1].loaded[0].rows_dropped == 2 and any(np.any(g.aperture & 64) for g in groups)


def test_a_flipped_byte_raises_and_frees_everything(ctx, seven, tmp_path, monkeypatch):
	blob, rec, ap, info = seven['made'][4]
	bad = bytearray(blob)
	bad[info['table_offset'] + 9 * info['row_bytes'] + info['columns']['FLUX_ERR'] + 5] ^= 0x04
	path = fc.write(tmp_path / 'flipped_tp.fits', bytes(bad))
	files = list(seven['files'])
	files[4] = path
	# every allocation and release on ctx, device and page-locked, counted at the C entries
	live = count_allocations(ctx, monkeypatch)
	with pytest.raises(ffi.ChecksumError, match=r'flipped_tp\.fits: HDU 1'):
		tpf.load_tpf_groups(ctx, files)
	assert live == {'device': 0, 'host': 0}, live
	# the counter counts: a good load holds 3 cubes per bucket and per sub-group until it is freed
	groups, index = tpf.load_tpf_groups(ctx, seven['files'])
	assert live == {'device': 12, 'host': 0}, live
	for g in groups:
		g.free()
	assert live == {'device': 0, 'host': 0}, live
	assert all(c is None for g in groups for c in g.cubes.values())
	monkeypatch.undo()
	groups, index = tpf.load_tpf_groups(ctx, files, verify=False)              # unverified, the flipped file loads
	flipped = np.frombuffer(bytes(bad), dtype=rec.dtype, count=len(rec), offset=info['table_offset'])
	got = groups[index[4][0]].cubes['images_err'].to_host()[index[4][1]].view('uint32')
	assert np.array_equal(got, tc.host_cube(flipped, 'FLUX_ERR')) and int((got != tc.host_cube(rec, 'FLUX_ERR')).sum()) == 1
	for g in groups:
		g.free()
