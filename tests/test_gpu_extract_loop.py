# -*- coding: utf-8 -*-
"""
The streamed extraction loop of the fused per-target kernel (``extract_small_stream``, csrc/aperture_dev.h) at its edges:
mask sizes around the groups of 8 of the pairwise leaf (tail only, exactly one group, groups plus a tail, the list limit of
128), cadence counts around the vector width and the 128 cadences of a wavefront's pass, special values in the in-mask data,
and a stamp whose CCD origin is 2^30 (the centroid terms are fused only where the product column * weight is exact).

Both device paths -- ``tp_aperture_photometry_from_sumimage`` (mask + streamed extraction in one launch) and ``tp_k2p2_masks``
+ ``tp_aperture_extract`` (the stand-alone kernels, which keep the two-operation centroid terms) -- are compared with
``oracle/aperture.py`` the way ``tests/test_gpu_aperture.py`` compares the same columns: the float32 sums (flux, flux_err,
flux_background) bit for bit, the float64 centroids to 1e-12 relative with the same NaN pattern; and with each other byte for
byte.

The masks: a sum image of noise alone has no K2P2 mask, so the plugin falls back to the minimum aperture (3 x 3 around the
target, AND the pixels the ``aperture`` image marks as collected) -- 1, 7, 8 or 9 pixels by the aperture image; a plateau of
16 / 17 pixels and a broad star give the K2P2 masks of 16, 17 and 128 pixels.  The sizes are asserted on the oracle's masks.
"""
import types
import numpy as np
import pytest

T_VALUES = (1, 2, 127, 128, 129, 131)
MODES = ('subtract+series', 'series', 'cube')
N_SPECIALS = 6
BIG_ORIGIN = 2**30


def _noise(H, W, seed):
	return 100.0 + np.random.default_rng(seed).normal(0, 1.0, (H, W))


def _plateau(H, W, pixels, centre, seed):
	S = _noise(H, W, seed)
	for (r, c) in pixels:
		S[r, c] = 5000.0 - 25.0 * np.hypot(r - centre[0], c - centre[1])
	return S


def _star(H, W, seed):
	yy, xx = np.mgrid[0:H, 0:W]
	return _noise(H, W, seed) + 139.24766500838336 * np.exp(-0.5 * (((yy - 7.0) / 2.0)**2 + ((xx - 7.0) / 2.6)**2))


def _aperture(H, W, tr, tc, n):
	"""Aperture image whose collected pixels leave ``n`` of the 3 x 3 minimum aperture around (tr, tc)."""
	ap = np.ones((H, W), dtype='int32')
	box = [(r, c) for r in range(tr - 1, tr + 2) for c in range(tc - 1, tc + 2) if (r, c) != (tr, tc)]
	for (r, c) in box[:9 - n]:
		ap[r, c] = 0
	return ap


def _cases(H, W):
	"""[(sum image, target (row, col) in the stamp, aperture image, stamp origin, expected mask size or None)]"""
	tr, tc = H // 2, W // 2
	full = np.ones((H, W), dtype='int32')
	cases = [(_noise(H, W, 13 + n), (tr, tc), _aperture(H, W, tr, tc, n), (100, 200), n) for n in (1, 7, 8, 9)]
	if (H, W) == (15, 15):
		blk = [(r, c) for r in range(6, 10) for c in range(6, 10)]
		cases.append((_plateau(H, W, blk, (7.0, 7.0), 2), (7, 7), full, (100, 200), 16))
		cases.append((_plateau(H, W, blk + [(10, 7)], (7.0, 7.0), 2), (7, 7), full, (100, 200), 17))
		cases.append((_star(H, W, 1), (7, 7), full, (100, 200), 128))
		# CCD origin 2^30: the target sits on the stamp's first pixel so that its catalogue position is a float32 number
		corner = [(r, c) for r in range(0, 4) for c in range(0, 4)]
		cases.append((_plateau(H, W, corner, (0.0, 0.0), 3), (0, 0), full, (BIG_ORIGIN, BIG_ORIGIN), None))
	cases.append((_noise(H, W, 30), (tr, tc), full, (100, 200), 9))    # (takes the all-NaN background series)
	return cases


class Batch(object):
	"""The targets of one stamp size: sum images, metadata, and the oracle's masks (computed once, shared by every test)."""

	def __init__(self, H, W):
		from oracle import aperture as oap
		self.H, self.W = H, W
		cases = _cases(H, W)
		self.n = Nt = len(cases)
		self.expected = [c[4] for c in cases]
		self.sumimage = np.stack([c[0] for c in cases])
		self.aperture = np.stack([c[2] for c in cases])
		tr = np.array([c[1][0] for c in cases]); tc = np.array([c[1][1] for c in cases])
		r0 = np.array([c[3][0] for c in cases], dtype='int64'); c0 = np.array([c[3][1] for c in cases], dtype='int64')
		self.stamps = np.column_stack((r0, r0 + H, c0, c0 + W)).astype('int32')
		self.target_pos_row = (r0 + tr).astype('float64')
		self.target_pos_column = (c0 + tc).astype('float64')
		self.target_tmag = np.full(Nt, 10.0)
		self.target_starid = (np.arange(Nt, dtype='int64') + 1) * 10
		self.cat_offsets = np.arange(Nt + 1, dtype='int64')
		self.catalog = {'starid': self.target_starid.copy(), 'tmag': np.full(Nt, 10.0, dtype='float32'),
			'row': self.target_pos_row.astype('float32'), 'column': self.target_pos_column.astype('float32'),
			'row_stamp': tr.astype('float32'), 'column_stamp': tc.astype('float32')}
		assert np.array_equal(self.catalog['row'].astype('float64'), self.target_pos_row)   # (exact in float32, 2^30 included)
		# the oracle's masks do not depend on the cubes: one cadence of ones is enough to get them
		one = np.ones((H, W, 1), dtype='float32')
		self.ref = [oap.do_photometry(self.sumimage[i], one, one, one, tuple(self.stamps[i]), self.target_pos_row[i], self.target_pos_column[i],
			self.target_tmag[i], self.target_starid[i], self.catalog_of(i), self.aperture[i]) for i in range(Nt)]

	def catalog_of(self, i):
		return {k: v[i:i + 1] for k, v in self.catalog.items()}

	def mask(self, i):
		return self.ref[i]['mask']

	def cubes(self, T, mode):
		"""raw images, errors, background series (Nt, T) and background cube with the special values; deterministic per (T, mode)."""
		Nt, H, W = self.n, self.H, self.W
		rng = np.random.default_rng(1000 + T)
		raw = rng.normal(300.0, 40.0, (Nt, H, W, T)).astype('float32')
		err = np.sqrt(np.abs(raw) + 50.0).astype('float32')
		ser = rng.normal(100.0, 3.0, (Nt, T)).astype('float32')
		cube = (ser[:, None, None, :] + rng.normal(0, 1.0, (Nt, H, W, T))).astype('float32')
		sub = (mode == 'subtract+series')
		for i in range(Nt):
			m = self.mask(i)
			pr, pc = np.argwhere(m)[len(np.argwhere(m)) // 2]       # a pixel of the mask
			# (special, cadence): all six at cadences of their own; with one or two cadences the targets take turns
			todo = [(s, (i + s) % T) for s in range(N_SPECIALS)] if T >= 8 else [((i + k) % N_SPECIALS, k) for k in range(T)]
			for s, k in todo:
				if s == 0:      # every pixel NaN
					raw[i, :, :, k] = np.nan
				elif s == 1:    # every pixel zero (after the subtraction)
					raw[i, :, :, k] = ser[i, k] if sub else 0.0
				elif s == 2:    # negative values and a -0.0 (x - y is -0.0 only for x = -0.0, y = +0.0)
					if sub:
						ser[i, k] = 0.0
					raw[i, :, :, k] = -np.abs(raw[i, :, :, k]) - 1
					raw[i, pr, pc, k] = -0.0
				elif s == 3:    # one pixel NaN
					raw[i, pr, pc, k] = np.nan
				elif s == 4:
					raw[i, pr, pc, k] = np.inf
				elif s == 5:    # background NaN: the series' entry, a pixel of the cube and a whole cadence of the cube's in-mask pixels
					ser[i, k] = np.nan
					cube[i, pr, pc, k] = np.nan
					cube[i, :, :, (k + 1) % T][m] = np.nan
		ser[Nt - 1, :] = np.nan    # one series that is all NaN (the last target repeats a mask size for this)
		return raw, err, ser, cube

	def reference(self, T, mode):
		from oracle import aperture as oap
		raw, err, ser, cube = self.cubes(T, mode)
		out = []
		for i in range(self.n):
			series = np.broadcast_to(ser[i][None, None, :], raw[i].shape)
			img = (raw[i] - series).astype('float32') if mode == 'subtract+series' else raw[i]
			bkg = cube[i] if mode == 'cube' else series
			out.append(oap.extract(img, err[i], bkg, self.mask(i), tuple(self.stamps[i])))
		return out


_BATCHES = {}


def _batch(H, W):
	if (H, W) not in _BATCHES:
		_BATCHES[(H, W)] = Batch(H, W)
	return _BATCHES[(H, W)]


@pytest.mark.parametrize("H,W", [(15, 15), (5, 7)])
def test_oracle_cases_are_comparable(H, W):
	"""No GPU: the oracle gives a mask of the intended size for every target and light curves with finite and NaN entries in
	every column, so that the device comparison below skips nothing."""
	b = _batch(H, W)
	sizes = []
	for i in range(b.n):
		assert 'mask' in b.ref[i], (i, b.ref[i]['errors'])
		n = int(b.mask(i).sum())
		sizes.append(n)
		if b.expected[i] is not None:
			assert n == b.expected[i], (i, n, b.expected[i])
		else:
			assert 8 < n <= 128 and n % 8 != 0, n         # the 2^30 target: full groups and a tail
	assert set(sizes) >= ({1, 7, 8, 9, 16, 17, 128} if (H, W) == (15, 15) else {1, 7, 8, 9})
	for T in T_VALUES:
		for mode in MODES:
			ref = b.reference(T, mode)
			for col in ('flux', 'flux_err', 'flux_background', 'pos_centroid'):
				a = np.stack([r[col] for r in ref])
				assert a.shape[:2] == (b.n, T)
				assert np.isfinite(a).any(), (T, mode, col)
			if T >= 8:
				flux = np.stack([r['flux'] for r in ref])
				assert np.isnan(flux).any() and np.isinf(flux).any() and (flux < 0).any()
				assert np.isnan(np.stack([r['flux_background'] for r in ref])).any()


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _device(ctx, b, T, mode):
	"""(fused path, stand-alone path): dicts of host arrays."""
	from photometry_amd import engine, pipeline
	from photometry_amd.device import DeviceCube
	raw, err, ser, cube = b.cubes(T, mode)
	img, imerr = DeviceCube.from_host(ctx, raw), DeviceCube.from_host(ctx, err)
	if mode == 'cube':
		bkg, subtract = DeviceCube.from_host(ctx, cube), None
	else:
		serp = np.zeros((b.n, img.t_pitch), dtype='float32')
		serp[:, :T] = ser
		bkg = ctx.array(serp)
		subtract = bkg if mode == 'subtract+series' else None
	scene = types.SimpleNamespace(quality=np.zeros(T, dtype='int32'), time=1325.0 + np.arange(T) / 48.0, stamps=b.stamps, cat_offsets=b.cat_offsets,
		catalog=b.catalog, target_pos_row=b.target_pos_row, target_pos_column=b.target_pos_column, target_tmag=b.target_tmag,
		target_starid=b.target_starid, aperture=b.aperture)
	batch = pipeline.ApertureBatch(ctx, scene, cubes={'images': img, 'images_err': imerr, 'backgrounds': None})
	out = []
	for fused in (True, False):
		work = pipeline.ApertureWork(ctx, batch)
		work.sumimage = ctx.array(b.sumimage)
		if fused:
			engine.aperture_photometry(ctx, batch, work, subtract=subtract, backgrounds=bkg, sumimage_given=True)
		else:
			engine.k2p2_masks(ctx, batch, work)
			engine.aperture_extract(ctx, img, imerr, bkg, work.mask, batch.stamps, status=work.status, out=work.lc, subtract=subtract)
		ctx.sync()
		res = work.lc.to_host()
		res['mask'], res['status'] = work.mask.to_host(), work.status.to_host()
		out.append(res)
	return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", T_VALUES)
@pytest.mark.parametrize("H,W", [(15, 15), (5, 7)])
def test_extract_loop_edges(ctx, H, W, T, mode):
	b = _batch(H, W)
	ref = b.reference(T, mode)
	fused, alone = _device(ctx, b, T, mode)
	for name, lc in (('fused', fused), ('stand-alone', alone)):
		for i in range(b.n):
			tag = f"{name} target {i} M={int(b.mask(i).sum())}"
			# (the status is the contamination step's, which this file is not about: the reference finds the target in its mask by
			# float32 arithmetic on CCD coordinates, np.round(row) + 1, which is not exact at 2^30, and the oracle restates that)
			if b.stamps[i].max() < 2**24:
				assert int(lc['status'][i]) == b.ref[i]['status'], tag
			np.testing.assert_array_equal(lc['mask'][i].astype(bool), b.mask(i), err_msg=tag)
			np.testing.assert_array_equal(lc['flux'][i], ref[i]['flux'], err_msg="flux " + tag)
			np.testing.assert_array_equal(lc['flux_err'][i], ref[i]['flux_err'], err_msg="flux_err " + tag)
			np.testing.assert_array_equal(lc['flux_background'][i], ref[i]['flux_background'], err_msg="bkg " + tag)
			np.testing.assert_allclose(lc['pos_centroid'][i], ref[i]['pos_centroid'], rtol=1e-12, equal_nan=True, err_msg=tag)
			np.testing.assert_array_equal(np.isnan(lc['pos_centroid'][i]), np.isnan(ref[i]['pos_centroid']), err_msg=tag)
	# the two device paths: byte for byte
	for col in ('flux', 'flux_err', 'flux_background', 'centroid_col', 'centroid_row'):
		assert fused[col].tobytes() == alone[col].tobytes(), col
	assert fused['mask'].tobytes() == alone['mask'].tobytes()
