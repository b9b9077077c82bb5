# -*- coding: utf-8 -*-
"""
Shared by tests/test_extract_variants_host.py (no GPU) and tests/test_gpu_extract_variants.py: the inputs, the oracle's side and
the device runs of the tests that take ``tp_aperture_fused_kernel`` (csrc/fused.hip) through every instantiation and
``extract_small_stream`` (csrc/aperture_dev.h) through both of its forms.

The seam.  After the mask is built the fused kernel lays the extraction's pixel table (``20 * round_up(M, 8)`` bytes for a mask of
``M`` pixels) at the start of its LDS block and keeps the mask's pixel list at ``k.lab``; the floats in between are the ``room``
in which a target's subtracted / background series are staged once.  A target whose series do not fit (``need > room``, where
``need`` is the number of DISTINCT series times the cadence count rounded up to the width of the vector loads) re-reads them from
HBM with every pixel group instead: other load buffers, two pixels at a time instead of four.  Which form ran cannot be seen from
outside, so the rule is restated here (``offset_of_lab``, ``room``, ``staged``), held to the kernel's own ``k2p2::shared_carve`` by
the CPU test, and every cadence count of the seam tests is derived from it: a change of the LDS plan moves them along.
"""
import ctypes
import functools
import types
import numpy as np

#: (H, W) of the stamps of the seam tests; the hand-made sum images are those of tests/test_gpu_extract_loop.py
SEAM_STAMPS = ((15, 15), (5, 7))
#: the three modes of tests/test_gpu_extract_loop.py plus a subtracted series that is ANOTHER array than the background series
SEAM_MODES = ('subtract+series', 'series', 'cube', 'subtract+own series')
#: bytes the light-curve arrays are prefilled with; their pitch is the cadence count + OUT_PAD
OUT_FILL, OUT_PAD = 0xA5, 5


def round_up(n, m):
	return (int(n) + m - 1) // m * m


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------

def offset_of_lab(H, W):
	"""Byte offset of ``k.lab`` in the work arrays of an ``H x W`` stamp (k2p2_core.h: shared_layout / shared_carve): S, tmp
	[Pa doubles each] and red [64] come first, then -- in the region the phases share -- Z, dist [Pa each] and hval."""
	Pa = max(H * W, 64)
	off_region = (2 * Pa + 64) * 8
	hval_len = max(Pa // 2 + 1, 64)
	return off_region + (2 * Pa + hval_len) * 8


def hostsim_offset_of_lab(H, W):
	"""The same offset from the kernel's own header (tests/hostsim/k2p2_hostsim.cpp)."""
	import k2p2_common
	lib = k2p2_common.build_hostsim()
	lib.hostsim_k2p2_lab_offset.restype = ctypes.c_longlong
	return int(lib.hostsim_k2p2_lab_offset(ctypes.c_int(H), ctypes.c_int(W)))


def room(H, W, M):
	"""Floats between the end of the pixel table of a mask of ``M`` pixels and the mask's pixel list."""
	return (offset_of_lab(H, W) - 20 * round_up(M, 8)) // 4


def staged(H, W, M, T, vec, n_series):
	"""Does a target take the LDS-staged form?  ``n_series``: distinct series arrays (0: none, never staged)."""
	need = n_series * round_up(T, vec)
	return n_series > 0 and 0 < need <= room(H, W, M)


def n_series(mode):
	"""Distinct series arrays a mode hands to the kernel."""
	return {'cube': 0, 'none': 0, 'series': 1, 'subtract+series': 1, 'subtract+none': 1, 'subtract+cube': 1, 'subtract+own series': 2}[mode]


def pitches(T, aligned):
	"""(pitch of the cubes, pitch of the series) in floats.  Aligned: the 32-float padding of DeviceCube.  Unaligned: an ODD cube pitch
	(the cadence count itself where that is odd: no padding at all) and an odd series pitch, either of which sends the entries to
	their scalar kernels (VEC 1)."""
	if aligned:
		return round_up(T, 32), round_up(T, 32)
	return T | 1, (T | 1) + 2


def vec_of(aligned):
	return 2 if aligned else 1


# ---- section 2: the hand-made masks of tests/test_gpu_extract_loop.py at the seam -------------------------------------------------------

def seam_batch(H, W):
	import test_gpu_extract_loop as loop
	return loop._batch(H, W)


def mask_sizes(b):
	return [int(b.mask(i).sum()) for i in range(b.n)]


def seam_rooms(b):
	"""The distinct rooms among the batch's masks, ascending."""
	return sorted({room(b.H, b.W, M) for M in mask_sizes(b)})


def seam_counts(b, mode):
	"""Cadence counts around every seam of the batch: R - 1 .. R + 2 for each distinct room R; around R / 2 where two arrays are staged."""
	div = 2 if n_series(mode) == 2 else 1
	return sorted({R // div + d for R in seam_rooms(b) for d in (-1, 0, 1, 2)})


def seam_cases():
	"""[(H, W, T, mode)] of the seam tests."""
	return [(H, W, T, mode) for (H, W) in SEAM_STAMPS for mode in SEAM_MODES for T in seam_counts(seam_batch(H, W), mode)]


def seam_cubes(b, T, mode):
	"""dict(raw, err, sub, ser, cube): the cubes of ``Batch.cubes`` (special values in the in-mask data); ``sub`` / ``ser`` are the
	subtracted and the background series ``(Nt, T)`` or None, ``cube`` the background cube or None."""
	raw, err, ser, cube = b.cubes(T, 'subtract+series' if mode.startswith('subtract') else mode)
	d = dict(raw=raw, err=err, sub=None, ser=None, cube=None)
	if mode == 'cube':
		d['cube'] = cube
	elif mode == 'series':
		d['ser'] = ser
	elif mode == 'subtract+series':
		d['sub'] = d['ser'] = ser
	else:
		assert mode == 'subtract+own series'
		d['sub'] = ser
		d['ser'] = own_series(b.n, T, ser)
	return d


def own_series(Nt, T, sub):
	"""A background series with other values and other NaN entries than the subtracted one."""
	own = np.random.default_rng(5000 + T).normal(80.0, 2.0, (Nt, T)).astype('float32')
	for i in range(Nt):
		own[i, (3 * i + 7) % T] = np.nan
	own[0, :] = np.nan
	assert not np.array_equal(np.isnan(own), np.isnan(sub))
	return own


def reference(b, d):
	"""The oracle's extraction of every target from the cubes ``d`` with the oracle's masks."""
	from oracle import aperture as oap
	out = []
	for i in range(b.n):
		raw = d['raw'][i]
		img = raw if d['sub'] is None else (raw - d['sub'][i][None, None, :]).astype('float32')
		if d['cube'] is not None:
			bkg = d['cube'][i]
		else:
			bkg = None if d['ser'] is None else np.broadcast_to(d['ser'][i][None, None, :], raw.shape)
		out.append(oap.extract(img, d['err'][i], bkg, b.mask(i), tuple(b.stamps[i])))
	return out


# ---- section 4: masks above 128 pixels ---------------------------------------------------------------------------------------------------

BIG_STAMP = (21, 21)
BIG_T = (51, 130)
BIG_MODES = ('series', 'subtract+series', 'subtract+own series', 'subtract+none')
#: (amplitude, width along the rows, width along the columns) of a Gaussian on noise, and the size of the oracle's mask
BIG_STARS = ((100.0, 1.9, 2.4, 130), (80.0, 1.9, 2.6, 136), (139.24766500838336, 2.2, 2.6, 187), (300.0, 3.0, 3.5, 259), (1000.0, 4.0, 4.5, 275))


class CaseBatch(object):
	"""``test_gpu_extract_loop.Batch`` for sum images of one's own: the targets' metadata and the oracle's masks, computed once."""

	def __init__(self, H, W, sumimages, origin=(100, 200)):
		from oracle import aperture as oap
		self.H, self.W = H, W
		self.n = Nt = len(sumimages)
		self.sumimage = np.stack(sumimages)
		self.aperture = np.ones((Nt, H, W), dtype='int32')
		tr, tc = np.full(Nt, H // 2), np.full(Nt, W // 2)
		r0 = np.full(Nt, origin[0], dtype='int64'); c0 = np.full(Nt, origin[1], dtype='int64')
		self.stamps = np.column_stack((r0, r0 + H, c0, c0 + W)).astype('int32')
		self.target_pos_row = (r0 + tr).astype('float64')
		self.target_pos_column = (c0 + tc).astype('float64')
		self.target_tmag = np.full(Nt, 10.0)
		self.target_starid = (np.arange(Nt, dtype='int64') + 1) * 10
		self.cat_offsets = np.arange(Nt + 1, dtype='int64')
		self.catalog = {'starid': self.target_starid.copy(), 'tmag': np.full(Nt, 10.0, dtype='float32'),
			'row': self.target_pos_row.astype('float32'), 'column': self.target_pos_column.astype('float32'),
			'row_stamp': tr.astype('float32'), 'column_stamp': tc.astype('float32')}
		one = np.ones((H, W, 1), dtype='float32')
		self.ref = [oap.do_photometry(self.sumimage[i], one, one, one, tuple(self.stamps[i]), self.target_pos_row[i], self.target_pos_column[i],
			self.target_tmag[i], self.target_starid[i], self.catalog_of(i), self.aperture[i]) for i in range(Nt)]

	def catalog_of(self, i):
		return {k: v[i:i + 1] for k, v in self.catalog.items()}

	def mask(self, i):
		return self.ref[i]['mask']


@functools.lru_cache(maxsize=None)
def big_batch():
	"""The targets of BIG_STARS and, last, one of noise alone (the minimum aperture of 9 pixels: the small-mask kernel and the big one
	share the launch)."""
	H, W = BIG_STAMP
	yy, xx = np.mgrid[0:H, 0:W]
	noise = 100.0 + np.random.default_rng(1).normal(0, 1.0, (H, W))
	images = [noise + a * np.exp(-0.5 * (((yy - 10.0) / sr)**2 + ((xx - 10.0) / sc)**2)) for (a, sr, sc, _n) in BIG_STARS]
	return CaseBatch(H, W, images + [noise])


def big_cubes(b, T, mode):
	"""dict(raw, err, sub, ser, cube) for the big masks: per target a cadence that is NaN in every pixel, one that is zero in every
	pixel (after the subtraction), a NaN and an inf in one mask pixel, and NaN entries of the background series."""
	Nt, H, W = b.n, b.H, b.W
	rng = np.random.default_rng(2000 + T)
	raw = rng.normal(300.0, 40.0, (Nt, H, W, T)).astype('float32')
	err = np.sqrt(np.abs(raw) + 50.0).astype('float32')
	ser = rng.normal(100.0, 3.0, (Nt, T)).astype('float32')
	has_sub = mode.startswith('subtract')
	for i in range(Nt):
		pr, pc = np.argwhere(b.mask(i))[int(b.mask(i).sum()) // 2]
		raw[i, :, :, (i + 0) % T] = np.nan
		raw[i, :, :, (i + 1) % T] = ser[i, (i + 1) % T] if has_sub else 0.0
		raw[i, pr, pc, (i + 2) % T] = np.nan
		raw[i, pr, pc, (i + 3) % T] = np.inf
		raw[i, :, :, (i + 4) % T] = -np.abs(raw[i, :, :, (i + 4) % T])
	d = dict(raw=raw, err=err, sub=None, ser=None, cube=None)
	if has_sub:
		d['sub'] = ser
	if mode == 'subtract+own series':
		d['ser'] = own_series(Nt, T, ser)
	elif mode in ('series', 'subtract+series'):
		d['ser'] = ser
		for i in range(Nt):     # (where the same series is subtracted, the flux of that cadence is NaN as well)
			ser[i, (i + 5) % T] = np.nan
	return d


# ---- section 3: two small raw scenes through every instantiation -----------------------------------------------------------------------------

#: name -> make_scene's (targets, cadences, H, W, seed)
SCENES = {'11x11': (12, 37, 11, 11, 49), '7x7': (12, 64, 7, 7, 76)}
#: (subtract, background): the seven valid pairs
PAIRS = (('none', 'cube'), ('none', 'series'), ('none', 'none'), ('own', 'cube'), ('own', 'series'), ('own', 'none'), ('same', 'series'))
#: the shapes real data has (section 5): every target takes the HBM-series form
LONG_SCENES = {'ffi 10 min': (6, 3900, 11, 11, 5), 'seam of 15 x 15': (4, 2116, 15, 15, 6)}
TIME_SMOOTH = 3


@functools.lru_cache(maxsize=None)
def raw_scene(shape):
	from photometry_amd import simulate
	n, T, H, W, seed = shape
	s = simulate.make_scene(n, T, H, W, seed=seed)
	simulate.fill_cubes(s, with_raw=True)
	s.aperture = None
	return s


def oracle_jobs(s):
	"""The jobs of ``test_gpu_raw_chain._oracle_target`` for the targets of a raw scene."""
	return [(s.raw[i], s.raw_err[i], s.quality, TIME_SMOOTH, tuple(s.stamps[i]), s.target_pos_row[i], s.target_pos_column[i],
		s.target_tmag[i], s.target_starid[i], s.catalog_of(i), s.height, s.width) for i in range(s.n_targets)]


@functools.lru_cache(maxsize=None)
def oracle_chain(shape):
	"""The oracle-only chain (B*, B2, B3, A1, K2P2, A6) of every target of a raw scene, computed once."""
	from test_gpu_raw_chain import _oracle_target
	return [_oracle_target(job) for job in oracle_jobs(raw_scene(shape))]


def scene_series(shape):
	"""(same, own): the series of the instantiation tests, float32 ``(Nt, T)``.  ``same`` is the oracle's smoothed background
	series of the raw cube, subtracted AND reported in the raw step's configuration; ``own`` is another array with other values,
	subtracted where the background is a cube, a different series or absent."""
	same = np.stack([o['bkg'] for o in oracle_chain(shape)]).astype('float32')
	rng = np.random.default_rng(77)
	own = (same * np.float32(0.96) + rng.normal(0, 0.5, same.shape)).astype('float32')
	return same, own


def scene_inputs(shape, pair):
	"""dict(raw, err, sub, ser, cube) of a raw scene for one (subtract, background) pair."""
	s = raw_scene(shape)
	same, own = scene_series(shape)
	subtract, background = pair
	d = dict(raw=s.raw, err=s.raw_err, sub=None, ser=None, cube=None)
	if subtract != 'none':
		d['sub'] = same if subtract == 'same' else own
	if background == 'series':
		d['ser'] = same
	elif background == 'cube':
		d['cube'] = s.backgrounds
	return d


# ---- the device side -------------------------------------------------------------------------------------------------------------------------

def upload_cube(ctx, host, pitch):
	"""A float32 cube ``(Nt, H, W, T)`` on the device with ``pitch`` floats per series; the padding is NaN."""
	from photometry_amd.device import DeviceCube
	host = np.ascontiguousarray(host, dtype='float32')
	Nt, H, W, T = host.shape
	d = DeviceCube(ctx, Nt, T, H, W, t_pitch=pitch)
	d.data.fill_bytes(0xFF)
	ctx._check(ctx.lib.tp_upload_cube(ctx.handle, d.ptr, pitch, host.ctypes.data, T, Nt * H * W, T))
	return d


def upload_series(ctx, host, pitch):
	"""Float32 series ``(Nt, T)`` on the device as ``(Nt, pitch)``; the padding is NaN."""
	Nt, T = host.shape
	p = np.full((Nt, pitch), np.nan, dtype='float32')
	p[:, :T] = host
	return ctx.array(p)


class Inputs(object):
	"""The device-resident inputs of one run: cubes, series (``sub`` and ``ser`` are ONE device array where they are one host array)."""

	def __init__(self, ctx, d, aligned):
		T = d['raw'].shape[3]
		cpitch, spitch = pitches(T, aligned)
		self.T, self.aligned = T, aligned
		self.img, self.err = upload_cube(ctx, d['raw'], cpitch), upload_cube(ctx, d['err'], cpitch)
		self.sub = None if d['sub'] is None else upload_series(ctx, d['sub'], spitch)
		if d['cube'] is not None:
			self.bkg = upload_cube(ctx, d['cube'], cpitch)
		elif d['ser'] is None:
			self.bkg = None
		else:
			self.bkg = self.sub if d['ser'] is d['sub'] else upload_series(ctx, d['ser'], spitch)
		for a in (self.img, self.err, self.sub, self.bkg):
			assert a is None or a.ptr % 16 == 0         # (the alignment is the pitch's alone)


def meta_scene(b, T):
	"""What ApertureBatch reads of a scene, for a hand-made batch."""
	return types.SimpleNamespace(quality=np.zeros(T, dtype='int32'), time=1325.0 + np.arange(T) / 48.0, stamps=b.stamps, cat_offsets=b.cat_offsets,
		catalog=b.catalog, target_pos_row=b.target_pos_row, target_pos_column=b.target_pos_column, target_tmag=b.target_tmag,
		target_starid=b.target_starid, aperture=b.aperture)


def new_work(ctx, batch, T):
	"""An ApertureWork whose light-curve arrays have a pitch above the cadence count and are prefilled with OUT_FILL."""
	from photometry_amd import engine, pipeline
	work = pipeline.ApertureWork(ctx, batch)
	work.lc = engine.LightCurves(ctx, batch.n_targets, T + OUT_PAD)
	work.lc.block.fill_bytes(OUT_FILL)
	return work


KEYS = ('sumimage', 'mask', 'status', 'flags', 'contamination', 'cat_in_mask', 'flux', 'flux_err', 'flux_background', 'centroid_col', 'centroid_row')
LC_COLUMNS = ('flux', 'flux_err', 'flux_background', 'centroid_col', 'centroid_row')


def collect(work):
	out = work.lc.to_host()          # (Nt, T + OUT_PAD) per column
	for k in ('sumimage', 'mask', 'status', 'flags', 'contamination', 'cat_in_mask'):
		out[k] = getattr(work, k).to_host()
	return out


def run(ctx, scene, inp, sumimage, path):
	"""One device run, dict of host arrays (``collect``).
	``sumimage``: a host array ``(Nt, H, W)`` that is given to the launch, or None: formed on the device from the images (and ``sub``).
	``path``: 'fused' (tp_aperture_photometry / _from_sumimage) or 'alone' (tp_sumimage, tp_k2p2_masks, tp_aperture_extract)."""
	from photometry_amd import engine, pipeline
	batch = pipeline.ApertureBatch(ctx, scene, cubes={'images': inp.img, 'images_err': inp.err, 'backgrounds': inp.bkg if hasattr(inp.bkg, 't_pitch') else None})
	work = new_work(ctx, batch, inp.T)
	if sumimage is not None:
		work.sumimage = ctx.array(np.ascontiguousarray(sumimage, dtype='float64'))
	if path == 'fused':
		engine.aperture_photometry(ctx, batch, work, subtract=inp.sub, backgrounds=inp.bkg, sumimage_given=sumimage is not None)
	else:
		if sumimage is None:
			engine.sumimage(ctx, inp.img, batch.quality, out=work.sumimage, subtract=inp.sub)
		engine.k2p2_masks(ctx, batch, work)
		engine.aperture_extract(ctx, inp.img, inp.err, inp.bkg, work.mask, batch.stamps, status=work.status, out=work.lc, subtract=inp.sub)
	ctx.sync()
	return collect(work)


def extract_with_mask(ctx, scene, inp, mask):
	"""``tp_aperture_extract`` alone on given masks ``(Nt, H, W)`` (no status): the light-curve columns on the host."""
	from photometry_amd import engine
	Nt = mask.shape[0]
	lc = engine.LightCurves(ctx, Nt, inp.T + OUT_PAD)
	lc.block.fill_bytes(OUT_FILL)
	dmask, dstamps = ctx.array(np.ascontiguousarray(mask, dtype='uint8')), ctx.array(np.ascontiguousarray(scene.stamps, dtype='int32'))
	engine.aperture_extract(ctx, inp.img, inp.err, inp.bkg, dmask, dstamps, status=None, out=lc, subtract=inp.sub)
	ctx.sync()
	return lc.to_host()


# ---- assertions ------------------------------------------------------------------------------------------------------------------------------

def check_padding(got, T, rows=None, tag=''):
	"""The light-curve arrays beyond the cadence count hold the prefilled bytes."""
	for col in LC_COLUMNS:
		pad = got[col][:, T:] if rows is None else got[col][rows, T:]
		assert pad.size and (pad.view('uint8') == OUT_FILL).all(), f"{col}: written beyond the cadence count {tag}"


def check_lightcurve(got, i, ref, T, tag):
	"""The columns of target ``i`` against the oracle's: the float32 sums bit for bit, the centroids to 1e-12 with the same NaNs."""
	np.testing.assert_array_equal(got['flux'][i, :T], ref['flux'], err_msg="flux " + tag)
	np.testing.assert_array_equal(got['flux_err'][i, :T], ref['flux_err'], err_msg="flux_err " + tag)
	np.testing.assert_array_equal(got['flux_background'][i, :T], ref['flux_background'], err_msg="flux_background " + tag)
	cen = np.stack((got['centroid_col'][i, :T], got['centroid_row'][i, :T]), axis=-1)
	np.testing.assert_allclose(cen, ref['pos_centroid'], rtol=1e-12, atol=0, equal_nan=True, err_msg="centroid " + tag)
	np.testing.assert_array_equal(np.isnan(cen), np.isnan(ref['pos_centroid']), err_msg="centroid NaNs " + tag)


def check_same_bytes(a, b, keys, tag):
	for k in keys:
		assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{k}: the two device paths differ {tag}"
