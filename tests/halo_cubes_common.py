# -*- coding: utf-8 -*-
"""
What the tests of Halo photometry on target pixel files share (tests/test_gpu_halo_cubes.py: the kernels of csrc/halo_cubes.hip
through the C ABI; tests/test_gpu_tpf_halo_switch.py: ``tessphot_tpfs(method=...)``; tests/test_tpf_halo_switch_host.py: the fixture
on the oracle alone):

* small per-target cubes on the device with a chosen pattern in the pads behind the last cadence, the three entries called directly,
  and the host restatement ``halo.build_problems`` / ``halo.pack`` they are held to;
* six target pixel files written from ``simulate`` scenes the way tests/test_gpu_tpf_batch.py::_write writes its files: two
  ``Tmag <= 6`` stars whose light reaches the stamp edge (one with a gap of more than half a day: two segments; one without: one
  segment), a ``Tmag <= 6`` star that stays inside its stamp, a ``Tmag <= 6`` star on the edge whose second segment has two fitted
  cadences (degenerate: "Halo optimization failed"), and two faint stars; four files of 11 x 11 x 70 and two of 9 x 13 x 70.
"""
import ctypes
import numpy as np
import ffi_common as fc
import tpf_common as tc

T = 70
VERSION = 6
#: the files: name -> (stamp height, width).  Their order is the input order of the tests.
FILES = ('edge_two_segments', 'edge_one_segment', 'inside', 'edge_degenerate', 'faint', 'faint_wide')
SWITCHING = (0, 1, 3)          # the files the edge-flux reason sends to Halo photometry
DEGENERATE = 3                 # ... of which this one ends in ERROR "Halo optimization failed"
TWO_SEGMENTS = (0, 3)


# ---- cubes for the kernels ----------------------------------------------------------------------------------------------------
def device_cube(ctx, images, pad):
	"""float32 ``(n, H, W, T)`` as a ``DeviceCube`` with ``t_pitch = round_up(T, 32)`` whose pads hold ``pad`` (never to be read)."""
	from photometry_amd.device import DeviceCube
	n, H, W, T_ = images.shape
	pitch = (T_ + 31) // 32 * 32
	full = np.full((n, H, W, pitch), pad, dtype='float32')
	full[..., :T_] = images
	cube = DeviceCube.from_host(ctx, full)
	assert cube.t_pitch == pitch
	cube.n_cad = T_
	return cube


def _ptr(a):
	return a.ctypes.data_as(ctypes.c_void_p)


def n_segments(seg):
	seg = np.asarray(seg)
	return int(seg.max()) + 1 if seg.size and seg.max() >= 0 else 0


def select_gather(ctx, cube, masks, segs, quality, n_seg=None, minflux=-100.0):
	"""``tp_halo_select_cubes`` and ``tp_halo_gather_cubes`` over the targets of ``cube``: per target a list over its segments of
	``{'pix', 'cad', 'fit', 'P'}`` (``P`` the padded block, ``None`` for the problems of a target with a segment without pixels),
	and ``cadpos`` ``(n, T)``."""
	from photometry_amd.engine import TESS_DEFAULT_BITMASK
	n, H, W, T_ = cube.n_targets, cube.height, cube.width, cube.n_cad
	HW = H * W
	segs = np.ascontiguousarray(segs, dtype='int32').reshape(n, T_)
	quality = np.ascontiguousarray(quality, dtype='int32').reshape(n, T_)
	n_seg = np.array([n_segments(s) for s in segs] if n_seg is None else n_seg, dtype='int32')
	prob_off = np.concatenate([[0], np.cumsum(n_seg)]).astype('int32')
	n_prob = int(prob_off[-1])
	geometry = (n, H, W, T_, cube.t_pitch)
	d_mask = ctx.array(np.ascontiguousarray(masks, dtype='uint8').reshape(n, HW))
	pix, cad, fit = ctx.empty((n_prob, HW), 'int32'), ctx.empty((n_prob, T_), 'int32'), ctx.empty((n_prob, T_), 'uint8')
	cadpos, counts = ctx.empty((n, T_), 'int32'), ctx.empty((2, n_prob), 'int32')
	ctx._check(ctx.lib.tp_halo_select_cubes(ctx.handle, cube.ptr, *geometry, d_mask.ptr, _ptr(prob_off), _ptr(segs), _ptr(quality), int(TESS_DEFAULT_BITMASK),
		float(minflux), pix.ptr, cad.ptr, fit.ptr, cadpos.ptr, counts.ptr, counts.ptr + 4 * n_prob))
	npix, ncad = counts.to_host()
	usable = np.array([np.all(npix[prob_off[i]:prob_off[i + 1]] >= 1) for i in range(n)])
	index = np.ascontiguousarray(np.flatnonzero(np.repeat(usable, n_seg)), dtype='int32')
	run_npix, run_ncad = np.ascontiguousarray(npix[index], dtype='int32'), np.ascontiguousarray(ncad[index], dtype='int32')
	pitch = (run_npix.astype('int64') + 3) // 4 * 4
	sizes = pitch * run_ncad
	offset = np.zeros(len(index), dtype='int64')
	offset[1:] = np.cumsum(sizes)[:-1]
	total = int(sizes.sum())
	# (both buffers start out as ones: the zeros of the padding have to be written)
	P = ctx.array(np.ones(max(total, 4), dtype='float32'))
	fitc = ctx.array(np.full(max(int(run_ncad.sum()), 1), 7, dtype='uint8'))
	ctx._check(ctx.lib.tp_halo_gather_cubes(ctx.handle, cube.ptr, *geometry, _ptr(prob_off), pix.ptr, cad.ptr, fit.ptr, len(index), _ptr(index), _ptr(offset),
		_ptr(run_npix), _ptr(run_ncad), P.ptr, fitc.ptr))
	hpix, hcad, hfit, hP, hfitc, hpos = pix.to_host(), cad.to_host(), fit.to_host(), P.to_host(), fitc.to_host(), cadpos.to_host()
	for a in (d_mask, pix, cad, fit, cadpos, counts, P, fitc):
		a.free()
	run = {int(q): r for r, q in enumerate(index)}
	co = np.concatenate([[0], np.cumsum(run_ncad)])
	out = []
	for i in range(n):
		per = []
		for q in range(prob_off[i], prob_off[i + 1]):
			block = None
			if q in run:
				r = run[q]
				block = hP[offset[r]:offset[r] + sizes[r]].reshape(run_ncad[r], pitch[r])
				assert np.array_equal(hfitc[co[r]:co[r + 1]], hfit[q, :ncad[q]]), 'the concatenated fit bytes are the selected ones'
			per.append({'pix': hpix[q, :npix[q]], 'cad': hcad[q, :ncad[q]], 'fit': hfit[q, :ncad[q]].astype(bool), 'P': block})
		out.append(per)
	return out, hpos


def hold_problems(dev, cadpos, images, masks, segs, quality, label):
	"""pix, cad, fit, counts equal and P bit-equal with zero padding, target by target against ``halo.build_problems``; ``cadpos`` is the
	position of every cadence in its problem's list."""
	from photometry_amd import halo
	for i, per in enumerate(dev):
		ref = halo.build_problems(images[i], quality[i], masks[i], np.asarray(segs[i]))
		assert len(ref) == len(per), (label, i)
		unusable = any(len(r.pix) == 0 for r in ref)
		want_pos = np.full(images.shape[3], -1)
		for k, (d, r) in enumerate(zip(per, ref)):
			where = f'{label}: target {i} segment {k}'
			np.testing.assert_array_equal(d['pix'], r.pix, err_msg=where)
			np.testing.assert_array_equal(d['cad'], r.cad, err_msg=where)
			np.testing.assert_array_equal(d['fit'], np.asarray(r.fit, dtype=bool), err_msg=where)
			want_pos[r.cad] = np.arange(len(r.cad))
			if unusable:
				assert d['P'] is None, where
				continue
			npix = len(r.pix)
			assert d['P'].shape == (len(r.cad), (npix + 3) // 4 * 4), where
			assert np.array_equal(d['P'][:, :npix].view('uint32'), r.P.view('uint32')), where
			assert not d['P'][:, npix:].view('uint32').any(), where
		np.testing.assert_array_equal(cadpos[i], want_pos, err_msg=f'{label}: target {i}')


def same_bits(a, b):
	a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
	return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view('uint8'), b.view('uint8'))


# ---- the six files ------------------------------------------------------------------------------------------------------------
def _times():
	"""A regular time axis (one segment) and one with a gap of 0.6 d in the middle (the gap rule of the split times finds it: the
	cadences are 0.02 d apart, so the gap lies between 30 % and 70 % of the span)."""
	regular = 1683.35 + np.arange(T) * 0.02
	gap = regular.copy()
	gap[T // 2:] += 0.6
	return regular, gap


def switch_scenes():
	"""The scenes and, per file of :data:`FILES`, ``(scene, target, starid offset, time, quality)``."""
	from photometry_amd import simulate
	wide = simulate.make_scene(2, T, 11, 11, seed=21, max_neighbours=0, tmag_range=(5.0, 5.9), sigma_psf=1.5, cadence_s=120.0)
	wide_b = simulate.make_scene(1, T, 9, 13, seed=22, max_neighbours=0, tmag_range=(5.0, 5.9), sigma_psf=3.0, cadence_s=120.0)
	inside = simulate.make_scene(1, T, 11, 11, seed=23, max_neighbours=1, tmag_range=(5.0, 5.9), cadence_s=120.0)
	faint = simulate.make_scene(1, T, 11, 11, seed=24, cadence_s=120.0)
	faint_b = simulate.make_scene(1, T, 9, 13, seed=25, cadence_s=120.0)
	for s in (wide, wide_b, inside, faint, faint_b):
		simulate.fill_cubes(s, nan_fraction=0.0)
	# the two stars of the 11 x 11 scene bleed along their columns over the whole stamp: 2 % of the star's flux per pixel of the trail
	for i in range(wide.n_targets):
		c = int(round(wide.star_params[i, 0, 1]))
		wide.images[i][:, c:c + 2, :] += np.float32(0.02 * wide.star_params[i, 0, 2])
	regular, gap = _times()
	few = np.zeros(T, dtype='int32')
	few[T // 2:T - 2] = 32                                                 # two fitted cadences are left behind the gap
	some = np.zeros(T, dtype='int32')
	some[[5, 50]] = 32
	return [(wide, 0, 100, gap, some), (wide_b, 0, 200, regular, None), (inside, 0, 300, regular, None), (wide, 1, 100, gap, few),
		(faint, 0, 400, regular, None), (faint_b, 0, 500, regular, None)]


def file_arrays(s, i, time, quality):
	"""What :func:`write_tpf` puts into the file of target ``i`` of scene ``s``: the three ``(T, H, W)`` cubes, the aperture image,
	``time`` and ``quality``."""
	h, w = s.height, s.width
	cubes = {'FLUX': np.moveaxis(s.images[i], 2, 0).copy(), 'FLUX_ERR': np.moveaxis(s.images_err[i], 2, 0).copy(), 'FLUX_BKG': np.moveaxis(s.backgrounds[i], 2, 0).copy()}
	ap = np.ones((h, w), dtype='int32')
	ap[3:8, 3:8] |= 2
	ap[4:7, 4:7] |= 8
	ap[:, :6] |= 32
	ap[:, 6:] |= 64
	ap[0, 0] &= ~1                                                         # a pixel never collected: NaN flux, bit 1 clear
	cubes['FLUX'][:, 0, 0] = np.nan
	cubes['FLUX_ERR'][:, 0, 0] = np.nan
	return cubes, ap, np.array(s.time if time is None else time, dtype='float64'), np.array(s.quality if quality is None else quality, dtype='int32')


def write_tpf(root, s, i, rng, starid_offset, time, quality):
	"""Target ``i`` of the scene ``s`` as a target pixel file (as tests/test_gpu_tpf_batch.py::_write); returns ``(path, starid)``."""
	cubes, ap, time, quality = file_arrays(s, i, time, quality)
	st = tuple(int(v) for v in s.stamps[i])
	n = s.n_cad
	scalars = {'TIME': time, 'TIMECORR': (3e-3 + 1e-5 * rng.normal(size=n)).astype('float32'), 'QUALITY': quality,
		'POS_CORR1': s.jitter[:, 0].astype('float32'), 'POS_CORR2': s.jitter[:, 1].astype('float32')}
	starid = int(s.target_starid[i]) + starid_offset
	blob, _, _, _ = tc.make_tpf(rng, s.height, s.width, n, crval1p=st[2] + 1, crval2p=st[0] + 1, aperture=ap, images=cubes, scalars=scalars,
		primary=dict(TICID=starid))
	return fc.write(root / ('tess2019199201929-s0014-%016d-0150-s_tp.fits' % starid), blob), starid


def catalog_and_targets(spec):
	"""One catalogue and one target list for all files, every scene's star numbers moved by its file's offset."""
	cat = {k: [] for k in ('starid', 'tmag', 'row', 'column')}
	tg = {k: [] for k in ('starid', 'tmag', 'row', 'column')}
	seen = set()
	for s, i, off, _, _ in spec:
		if id(s) in seen:
			continue
		seen.add(id(s))
		for k in ('tmag', 'row', 'column'):
			cat[k].append(s.catalog[k])
		cat['starid'].append(s.catalog['starid'] + off)
		tg['starid'].append(s.target_starid + off)
		tg['tmag'].append(s.target_tmag)
		tg['row'].append(s.target_pos_row)
		tg['column'].append(s.target_pos_column)
	return {k: np.concatenate(v) for k, v in cat.items()}, {k: np.concatenate(v) for k, v in tg.items()}


def write_switch_files(root):
	"""The six files; returns ``{'files', 'starid', 'catalog', 'targets', 'spec'}``."""
	rng = np.random.default_rng(71)
	spec = switch_scenes()
	made = [write_tpf(root, s, i, rng, off, time, quality) for s, i, off, time, quality in spec]
	cat, tg = catalog_and_targets(spec)
	return {'files': [m[0] for m in made], 'starid': [m[1] for m in made], 'catalog': cat, 'targets': tg, 'spec': spec}
