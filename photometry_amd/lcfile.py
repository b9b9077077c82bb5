# -*- coding: utf-8 -*-
"""
The light-curve file, ``tess…-tasoc_lc.fits.gz`` (FILEVER 1.5; BasePhotometry.save_lightcurve, BasePhotometry.py:1417-1730), for both
paths that produce one:

* :func:`lightcurve_hdus` -- every card and column of the file from plain inputs.  ``BasePhotometry.save_lightcurve``
  (photometry_amd/plugins.py) is a thin caller of it, one target at a time;
* :func:`save_lightcurves` (``BatchResults.save_lightcurves``) -- the files of a whole batch of the frames entry
  (``tessphot_frames``): the ``QUALITY`` column of every target from one launch on the region's pixel-flag stack
  (``FrameStack.stamp_flag_series``, csrc/stampflags.hip), the images cropped from the region's, bytes and gzip on a thread pool;
* :class:`FileInfo` -- what such a batch cannot know from its arguments (sector, camera, CCD, the input file's header, ...).

Building the bytes is host work: a file is 96 bytes per cadence against the 40 + 16 that cross the link as light curve and
``QUALITY``.  Compressing them is host work too by default (``compress='zlib'``) and dominates it;
``compress='device'`` hands the bytes of a window of files to the device's DEFLATE encoder instead (``deflate.gzip_many``, section 19).
With ``table='device'`` besides, the ``LIGHTCURVE`` table's data unit -- what grows with the series -- is written by a kernel straight
into the encoder's input with its DATASUM (:func:`lightcurve_pieces`, ``tp_lc_table_pack``, section 21) and the host builds headers
and the image HDUs only.
"""

import ctypes
import datetime
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
import numpy as np
from . import fitsio
from .fitsio import card
from .device import round_up
from ._lib import tp_lc_table_src
from .status import STATUS

#: PixelQualityFlags.BackgroundShenanigans / CorrectorQualityFlags.BackgroundShenanigans (photometry/quality.py:163, :85)
PIXEL_BACKGROUND_SHENANIGANS = 4
CORRECTOR_BACKGROUND_SHENANIGANS = 256
#: PROCVER card of the light-curve files this package writes
PROCVER = 'photometry_amd-0.2'
#: the most threads :func:`save_lightcurves` writes files with
MAX_WORKERS = 16
#: what ``compress=`` takes: gzip on the workers (the default: the bytes ``gzip.open`` writes), or DEFLATE on the device
COMPRESS = ('zlib', 'device')
#: what ``table=`` takes: the ``LIGHTCURVE`` table's data unit from numpy on the workers (the default), or written on the device straight
#: into the encoder's input with its DATASUM (``tp_lc_table_pack``, csrc/lctable.hip; needs ``compress='device'``)
TABLE = ('host', 'device')
#: bytes of a row of the ``LIGHTCURVE`` table (``NAXIS1``)
ROW_BYTES = 96
#: files whose bytes are held at a time with ``compress='device'``: built, compressed in batches, written, then the next window
DEVICE_WINDOW = 256


def _add_timings(timings, spent):
	for k, v in spent.items():
		if isinstance(v, dict):
			_add_timings(timings.setdefault(k, {}), v)
		else:
			timings[k] = timings.get(k, 0.0) + v


def _write_files(build, wanted, workers, compress, compresslevel, ctx, spent, table='host', shared=None):
	"""
	The files of the targets ``wanted``: ``build(i) -> (path, hdus, seconds)`` on ``workers`` threads, then the gzip member.
	``'zlib'``: the worker that built the bytes compresses and writes them (``fitsio.write``).  ``'device'``: per window of
	:data:`DEVICE_WINDOW` files the workers build the bytes, the calling thread -- the owner of ``ctx`` -- compresses them in batches
	(``deflate.gzip_many``), and the workers write the members.  Returns the paths in the order of ``wanted``; adds the seconds to
	``spent['build']`` and ``spent['gzip']`` (``'device'``: the wall time of the device path, its parts as ``deflate.gzip_many`` names
	them in ``spent['gzip_parts']``, and ``spent['write']`` for the files).  ``table='device'`` (with ``'device'``):
	``build(i) -> (path, LightcurvePieces, source, seconds)`` -- the host pieces of the file and the series its table is made of --, and
	the window's bytes are completed on the device before they are compressed from there (:func:`_pack_window`, which takes ``shared``
	and adds ``spent['table']`` and ``spent['place']``; ``deflate.gzip_device``).
	"""
	import time as _clock
	workers = min(MAX_WORKERS, os.cpu_count() or 1) if workers is None else max(1, min(MAX_WORKERS, int(workers)))
	wanted = [int(i) for i in wanted]
	serial = workers == 1 or len(wanted) <= 1

	def zlib_one(i):
		path, hdus, t_build = build(i)
		tb = _clock.perf_counter()
		fitsio.write(path, hdus, compresslevel=compresslevel)
		return path, t_build, _clock.perf_counter() - tb

	def build_one(i):
		path, hdus, t_build = build(i)
		return path, b''.join(hdus), t_build

	def write_one(job):
		tb = _clock.perf_counter()
		with open(job[0], 'wb') as fh:
			fh.write(job[1])
		return _clock.perf_counter() - tb

	if compress == 'zlib':
		if serial:
			done = [zlib_one(i) for i in wanted]
		else:
			with ThreadPoolExecutor(max_workers=workers) as pool:
				done = list(pool.map(zlib_one, wanted))
		for _path, t_build, t_gzip in done:
			spent['build'] += t_build
			spent['gzip'] += t_gzip
		return [d[0] for d in done]
	from . import deflate
	paths = []
	pool = None if serial else ThreadPoolExecutor(max_workers=workers)
	try:
		run = (lambda f, jobs: [f(j) for j in jobs]) if serial else (lambda f, jobs: list(pool.map(f, jobs)))
		for a in range(0, len(wanted), DEVICE_WINDOW):
			built = run(build if table == 'device' else build_one, wanted[a:a + DEVICE_WINDOW])
			spent['build'] += sum(b[-1] for b in built)
			parts = spent.setdefault('gzip_parts', {})
			if table == 'device':
				d_files, offsets = _pack_window(ctx, built, shared, spent)
				tb = _clock.perf_counter()
				try:
					members = deflate.gzip_device(ctx, d_files, offsets, parts=parts)
				finally:
					d_files.free()
			else:
				tb = _clock.perf_counter()
				members = deflate.gzip_many(ctx, [b[1] for b in built], parts=parts)
			spent['gzip'] += _clock.perf_counter() - tb
			spent['write'] = spent.get('write', 0.0) + sum(run(write_one, [(b[0], m) for b, m in zip(built, members)]))
			paths.extend(b[0] for b in built)
	finally:
		if pool is not None:
			pool.shutdown()
	return paths


def _check_table(table, compress):
	if table not in TABLE:
		raise ValueError(f"table must be one of {TABLE}, not {table!r}")
	if table == 'device' and compress != 'device':
		raise ValueError("table='device' needs compress='device': the table's bytes never exist on the host")


def _upload(ctx, block, nbytes):
	"""The first ``nbytes`` bytes (rounded up to 16) of the page-locked ``block`` into a new device array, queued on the context's stream."""
	words = round_up(max(int(nbytes), 16), 16) // 4
	d = ctx.empty(4 * words, 'uint8')
	ctx._check(ctx.lib.tp_upload_cube_async(ctx.handle, d.ptr, words, block.ptr, words, 1, words))
	return d


class _PackGroup(object):
	"""The files of a window whose tables one ``tp_lc_table_pack`` writes: one ``T``, one list of kept rows."""

	def __init__(self, T, rows):
		self.T, self.rows, self.members = int(T), rows, []


def _pack_window(ctx, built, shared, spent):
	"""
	The device work of one window of ``table='device'`` files.  ``built``: per file ``(path, LightcurvePieces, source, seconds)`` with
	``source`` a dict ``time, timecorr, cadenceno, pixel_quality`` (length ``T``), ``lc`` (five series of length ``T``: flux, flux_err,
	flux_background, centroid column, centroid row), ``quality`` (``T`` or None) and ``pos_corr`` (``(T, 2)`` or None); ``shared``: the
	four vectors when all files have the same (stride 0), else None.  Returns ``(device array of the files' bytes, offsets)`` with every
	file complete in it: the tables packed on the device (one launch per group of files with one ``T`` and one row list), the host
	pieces -- primary HDU, the table's header with the downloaded DATASUM, the image HDUs -- uploaded compactly and placed by one
	``tp_lc_place``.  ``spent``: ``table`` (upload, pack, download of the sums), ``build`` (the headers) and ``place`` are added to.
	"""
	import time as _clock
	lib = ctx.lib
	n = len(built)
	t0 = _clock.perf_counter()
	groups = {}
	for k, (_path, pieces, src, _t) in enumerate(built):
		key = (len(src['time']), pieces.rows.tobytes())
		groups.setdefault(key, _PackGroup(key[0], pieces.rows)).members.append(k)
	# the files' layout: front | table header | table data | back, every piece a multiple of 2880
	hdr_bytes = [fitsio._padded(80 * (len(fitsio.bintable_cards('LIGHTCURVE', b[1].columns, b[1].cards, len(b[1].rows))) + 3)) for b in built]
	unit = [fitsio._padded(ROW_BYTES * len(b[1].rows)) for b in built]
	sizes = [len(b[1].front) + h + u + len(b[1].back) for b, h, u in zip(built, hdr_bytes, unit)]
	offsets = np.zeros(n + 1, dtype='uint64')
	offsets[1:] = np.cumsum(sizes, dtype='uint64')
	table_at = [int(offsets[k]) + len(built[k][1].front) + hdr_bytes[k] for k in range(n)]
	# the sources of all groups in one page-locked block: per group the float64 arrays, then the int32 arrays
	plan, at = [], 0
	for g in groups.values():
		m, T = len(g.members), g.T
		vec = T if shared is not None else m * T
		has_q = any(built[k][2].get('quality') is not None for k in g.members)
		has_pc = any(built[k][2].get('pos_corr') is not None for k in g.members)
		list_rows = len(g.rows) != T
		lay = {'time': at, 'timecorr': at + 8 * vec, 'lc': at + 16 * vec}
		at += 16 * vec + 40 * m * T
		if has_pc:
			lay['pos_corr'] = at
			at += 16 * m * T
		lay['cadenceno'], lay['pixel_quality'] = at, at + 4 * vec
		at += 8 * vec
		if has_q:
			lay['quality'] = at
			at += 4 * m * T
		if list_rows:
			lay['rows'] = at
			at += 4 * len(g.rows)
		at = round_up(at, 16)
		plan.append((g, lay, vec))
	up = ctx.pinned_block(max(at, 16))
	d_src = d_files = d_sums = d_host = None
	host = sums_block = None
	try:
		buf = up.array
		for g, lay, vec in plan:
			m, T = len(g.members), g.T
			f8 = lambda name, count: buf[lay[name]:lay[name] + 8 * count].view('float64')   # noqa: E731
			i4 = lambda name, count: buf[lay[name]:lay[name] + 4 * count].view('int32')     # noqa: E731
			for name, view in (('time', f8), ('timecorr', f8), ('cadenceno', i4), ('pixel_quality', i4)):
				dst = view(name, vec)
				if shared is not None:
					dst[:] = shared[name]
				else:
					for j, k in enumerate(g.members):
						dst[j * T:(j + 1) * T] = built[k][2][name]
			lc = f8('lc', 5 * m * T).reshape(5, m, T)
			pc = f8('pos_corr', 2 * m * T).reshape(m, T, 2) if 'pos_corr' in lay else None
			q = i4('quality', m * T).reshape(m, T) if 'quality' in lay else None
			for j, k in enumerate(g.members):
				src = built[k][2]
				for p in range(5):
					lc[p, j] = src['lc'][p]
				if pc is not None:
					pc[j] = 0.0 if src.get('pos_corr') is None else src['pos_corr']
				if q is not None:
					q[j] = 0 if src.get('quality') is None else src['quality']
			if 'rows' in lay:
				i4('rows', len(g.rows))[:] = g.rows
		d_src = _upload(ctx, up, at)
		d_files = ctx.empty(max(int(offsets[-1]), 16), 'uint8')
		d_sums = ctx.empty(8 * n, 'uint8')
		order = []
		for g, lay, vec in plan:
			m, T = len(g.members), g.T
			stride = 0 if shared is not None else T
			base = d_src.ptr
			desc = tp_lc_table_src(base + lay['time'], stride, base + lay['timecorr'], stride, base + lay['cadenceno'], stride, base + lay['pixel_quality'], stride,
				base + lay['lc'], m * T, T, (base + lay['quality']) if 'quality' in lay else None, T, (base + lay['pos_corr']) if 'pos_corr' in lay else None, 2 * T)
			out_offsets = np.array([table_at[k] for k in g.members], dtype='uint64')
			ctx._check(lib.tp_lc_table_pack(ctx.handle, ctypes.byref(desc), (base + lay['rows']) if 'rows' in lay else None, len(g.rows), T, m, d_files.ptr,
				out_offsets.ctypes.data, d_files.nbytes, d_sums.ptr + 8 * len(order)))
			order.extend(g.members)
		sums_block = ctx.pinned_block(8 * n)
		ctx.download_async(sums_block, d_sums, nbytes=8 * n)
		ctx.sync()
		sums = np.array(sums_block.array[:8 * n].view('uint64'))
		t1 = _clock.perf_counter()
		spent['table'] = spent.get('table', 0.0) + t1 - t0
		# the host pieces, compact: front + table header (they touch in the file), then back
		datasum = dict(zip(order, (int(v) for v in sums)))
		pieces_bytes, seg = [], []
		at = 0
		for k, (_path, pieces, _src, _t) in enumerate(built):
			head = pieces.front + fitsio.bintable_header('LIGHTCURVE', pieces.columns, pieces.cards, len(pieces.rows), datasum[k])
			assert len(head) == len(pieces.front) + hdr_bytes[k]
			for blob, dst in ((head, int(offsets[k])), (pieces.back, table_at[k] + unit[k])):
				if blob:
					pieces_bytes.append(blob)
					seg.append((at, dst, len(blob)))
					at += len(blob)
		t2 = _clock.perf_counter()
		spent['build'] += t2 - t1
		host = ctx.pinned_block(max(at, 16))
		pos = 0
		for blob in pieces_bytes:
			host.array[pos:pos + len(blob)] = np.frombuffer(blob, dtype='uint8')
			pos += len(blob)
		d_host = _upload(ctx, host, at)
		seg = np.array(seg, dtype='uint64').reshape(-1, 3)
		so, do, ln = (np.ascontiguousarray(seg[:, c]) for c in range(3))
		ctx._check(lib.tp_lc_place(ctx.handle, d_host.ptr, d_host.nbytes, so.ctypes.data, do.ctypes.data, ln.ctypes.data, len(seg), d_files.ptr, d_files.nbytes))
		ctx.sync()                                    # (the page-locked blocks return to the pool below: their transfers are over)
		spent['place'] = spent.get('place', 0.0) + _clock.perf_counter() - t2
		out, d_files = d_files, None
		return out, offsets
	finally:
		for d in (d_src, d_sums, d_host, d_files):
			if d is not None:
				d.free()
		for block in (up, host, sums_block):
			if block is not None:
				ctx.pinned_release(block)


def weightmap_hdu(weightmap, shape, cards=()):
	"""The ``WEIGHTMAP`` binary table of Halo photometry (BasePhotometry.py:1673-1706): one row per segment."""
	npx = int(np.prod(shape))
	i32, disp = 'column format: signed 32-bit integer', 'column display format'
	wms = np.asarray(weightmap['weightmap'], dtype='float32').reshape(-1, shape[0], shape[1])
	columns = [
		{'name': 'CADENCENO1', 'format': 'J', 'array': np.asarray(weightmap['initial_cadence'], dtype='int32'), 'disp': 'I10',
			'comments': {'TTYPE': 'column title: first cadence number', 'TFORM': i32, 'TDISP': disp}},
		{'name': 'CADENCENO2', 'format': 'J', 'array': np.asarray(weightmap['final_cadence'], dtype='int32'), 'disp': 'I10',
			'comments': {'TTYPE': 'column title: last cadence number', 'TFORM': i32, 'TDISP': disp}},
		{'name': 'SAT_PIXELS', 'format': 'J', 'array': np.asarray(weightmap['sat_pixels'], dtype='int32'), 'disp': 'I10',
			'comments': {'TTYPE': 'column title: Saturated pixels', 'TFORM': i32, 'TDISP': disp}},
		{'name': 'WEIGHTMAP', 'format': f'{npx:d}E', 'array': wms, 'disp': 'E14.7', 'dim': (int(shape[1]), int(shape[0])),
			'comments': {'TTYPE': 'column title: Weightmap', 'TFORM': 'column format: image of 32-bit floating point', 'TDISP': disp,
				'TDIM': 'column dimensions: pixel aperture array'}},
	]
	return fitsio.bintable_hdu('WEIGHTMAP', columns, cards)


def ffi_aperture(sumimage, stamp, backgrounds_pixels_used=None, row0=0, col0=0):
	"""
	The aperture image of an FFI target (BasePhotometry.py:1033-1061): bit 1 where the sum image is finite, bits 32 .. 256 for the CCD
	output of the column, bit 4 where the pixel was used for the background (``backgrounds_pixels_used``: bool image whose pixel
	(0, 0) is CCD pixel ``(row0, col0)``).  ``stamp``: ``(r1, r2, c1, c2)`` of ``sumimage``.
	"""
	cols, _rows = np.meshgrid(np.arange(stamp[2] + 1, stamp[3] + 1, 1, dtype='int32'), np.arange(stamp[0] + 1, stamp[1] + 1, 1, dtype='int32'))
	ap = np.asarray(np.isfinite(sumimage), dtype='int32')
	ap[(45 <= cols) & (cols <= 556)] |= 32
	ap[(557 <= cols) & (cols <= 1068)] |= 64
	ap[(1069 <= cols) & (cols <= 1580)] |= 128
	ap[(1581 <= cols) & (cols <= 2092)] |= 256
	if backgrounds_pixels_used is not None: # pixels used for the background calculation (:1052-1061)
		ap[backgrounds_pixels_used[stamp[0] - row0:stamp[1] - row0, stamp[2] - col0:stamp[3] - col0]] |= 4
	return ap


def aperture_with_masks(aperture, phot_mask=None, position_mask=None):
	"""The ``APERTURE`` image of the file: bit 2 where the photometry mask lies, bit 8 where the position mask does (:1643-1649)."""
	mask = np.array(aperture, dtype='int32', copy=True)
	if phot_mask is not None:
		mask[np.asarray(phot_mask, dtype=bool)] |= 2
	if position_mask is not None:
		mask[np.asarray(position_mask, dtype=bool)] |= 8
	return mask


def image_cards(stamp, wcs_header=None):
	"""The cards of the image extensions without ``INHERIT``: the WCS of the stamp (:1651-1661) when ``wcs_header`` (a callable
	``stamp -> cards``) is given, else the stamp limits (``STAMP_*``)."""
	if wcs_header is not None:
		return [card(*c) for c in wcs_header(stamp)]
	return [card('STAMP_R1', int(stamp[0]), 'first CCD row of the stamp'), card('STAMP_R2', int(stamp[1]), 'last CCD row + 1'),
		card('STAMP_C1', int(stamp[2]), 'first CCD column of the stamp'), card('STAMP_C2', int(stamp[3]), 'last CCD column + 1')]


def lightcurve_filename(starid, sector, camera, ccd, cadence, data_rel, version):
	"""The reference's file name (:1708-1717)."""
	return (f'tess{int(starid):011d}-s{int(sector):03d}-{int(camera):d}-{int(ccd):d}-c{int(cadence):04d}'
		f'-dr{int(data_rel or 0):02d}-v{int(version):02d}-tasoc_lc.fits.gz')


def relative_filepath(path, output_folder, output_folder_base, input_folder=None):
	"""``details['filepath_lightcurve']``: relative to the input folder when the output lies inside it, else to the base output folder (:1722-1726)."""
	base = output_folder_base
	inp = input_folder if isinstance(input_folder, (str, bytes, os.PathLike)) else None
	if inp is not None and os.path.realpath(output_folder).startswith(os.path.realpath(inp)):
		base = os.path.abspath(inp)
	return os.path.relpath(path, base).replace('\\', '/')


def lightcurve_hdus(target, starid, sector, camera, ccd, cadence, data_rel, version, method, ticver, header, num_frm, n_readout,
	additional_headers, lightcurve, quality, sumimage, aperture, image_cards, weightmap=None):
	"""
	The HDUs of a light-curve file as byte strings (:func:`fitsio.write` joins them): primary header (:1463-1505), the ``LIGHTCURVE``
	binary table with the 14 columns and their units / display formats (:1507-1600), the time keywords of the table header
	(:1602-1641), the ``SUMIMAGE`` and ``APERTURE`` image extensions (:1643-1665) and, for a Halo target (``weightmap``: the dict of
	``halo.photometry``), the ``WEIGHTMAP`` table (:1673-1706); ``CHECKSUM`` / ``DATASUM`` in every HDU (:1720).

	``target``: dict with ``tmag`` and, optionally, ``ra_J2000, decl_J2000, pm_ra, pm_decl, teff``.  ``header``: the input file's
	(``CRMITEN, CRBLKSZ, CRSPOC``).  ``additional_headers``: key -> value or ``(value, comment)``, in order (K2P2 settings,
	``AP_CONT``, ``HALO_*``).  ``lightcurve``: columns ``time, timecorr, cadenceno, quality, flux, flux_err, flux_background`` of one
	length and ``pos_centroid, pos_corr`` ``(T, 2)``; ``quality`` (``QUALITY``, the photometry quality flags) has that length too.
	Rows without a finite time are dropped from every column (:1451-1452; upstream leaves ``QUALITY`` at its full length there, which
	no table can hold -- it is cut to the same rows).  ``aperture``: the ``APERTURE`` image with the mask bits already in it
	(:func:`aperture_with_masks`).  ``image_cards``: the cards of the two image extensions without ``INHERIT`` (:func:`image_cards`).
	"""
	indx = np.isfinite(np.asarray(lightcurve['time']))
	quality = np.asarray(quality)[indx]
	col = {k: np.asarray(lightcurve[k])[indx] for k in lightcurve.keys()}
	nan = np.full(len(col['time']), np.nan)
	arrays = {'TIME': col['time'], 'TIMECORR': col['timecorr'], 'CADENCENO': col['cadenceno'], 'FLUX_RAW': col['flux'], 'FLUX_RAW_ERR': col['flux_err'],
		'FLUX_BKG': col['flux_background'], 'FLUX_CORR': nan, 'FLUX_CORR_ERR': nan, 'QUALITY': quality, 'PIXEL_QUALITY': col['quality'],
		'MOM_CENTR1': col['pos_centroid'][:, 0], 'MOM_CENTR2': col['pos_centroid'][:, 1], 'POS_CORR1': col['pos_corr'][:, 0], 'POS_CORR2': col['pos_corr'][:, 1]}
	columns = [dict(c, array=arrays[c['name']]) for c in table_columns()]
	tcards = _time_cards(col['time'], cadence, header, num_frm, n_readout)
	return ([fitsio.primary_hdu(_primary_cards(target, starid, sector, camera, ccd, data_rel, version, method, ticver, header, additional_headers, weightmap is not None)),
		fitsio.bintable_hdu('LIGHTCURVE', columns, tcards)] + _image_hdus(sumimage, aperture, image_cards, weightmap))


#: what :func:`lightcurve_pieces` returns: ``front`` (the bytes before the table header: the primary HDU), ``columns`` and ``cards`` of the
#: ``LIGHTCURVE`` table (``fitsio.bintable_header('LIGHTCURVE', columns, cards, len(rows), datasum)`` is its header), ``rows`` (int32: the
#: kept cadences, rising) and ``back`` (the bytes behind the table's data unit: ``SUMIMAGE``, ``APERTURE`` and a Halo target's ``WEIGHTMAP``)
LightcurvePieces = namedtuple('LightcurvePieces', 'front columns cards rows back')


def lightcurve_pieces(target, starid, sector, camera, ccd, cadence, data_rel, version, method, ticver, header, num_frm, n_readout,
	additional_headers, time, sumimage, aperture, image_cards, weightmap=None):
	"""
	The light-curve file of :func:`lightcurve_hdus` without the ``LIGHTCURVE`` table's data unit and without the header that needs its
	``DATASUM``, for a table whose bytes are formed elsewhere (``tp_lc_table_pack``): a :data:`LightcurvePieces`.  The arguments are
	those of :func:`lightcurve_hdus` with ``time`` (the ``time`` column at its full length) in place of the columns;
	``front + bintable_header(...) + data unit + back`` is ``b''.join(lightcurve_hdus(...))``.
	"""
	time = np.asarray(time)
	rows = np.flatnonzero(np.isfinite(time)).astype('int32')
	return LightcurvePieces(
		fitsio.primary_hdu(_primary_cards(target, starid, sector, camera, ccd, data_rel, version, method, ticver, header, additional_headers, weightmap is not None)),
		table_columns(), _time_cards(time[rows], cadence, header, num_frm, n_readout), rows, b''.join(_image_hdus(sumimage, aperture, image_cards, weightmap)))


def _image_hdus(sumimage, aperture, image_cards, weightmap):
	"""``SUMIMAGE``, ``APERTURE`` and, for a Halo target, ``WEIGHTMAP``: the cards of the stamp, then INHERIT."""
	SumImage = np.asarray(sumimage, dtype='float64')
	icards = list(image_cards) + [card('INHERIT', True, 'inherit the primary header')]
	hdus = [fitsio.image_hdu('SUMIMAGE', SumImage, icards), fitsio.image_hdu('APERTURE', np.asarray(aperture, dtype='int32'), icards)]
	if weightmap is not None:
		hdus.append(weightmap_hdu(weightmap, SumImage.shape, icards))
	return hdus


def _primary_cards(target, starid, sector, camera, ccd, data_rel, version, method, ticver, header, additional_headers, has_weightmap):
	"""The cards of the primary header (:1463-1505)."""
	tgt = target
	undef = fitsio.Undefined()

	def opt(key): # "undefined" card for a missing or zero value, as upstream writes it (:1487-1490)
		v = tgt.get(key)
		return undef if not v else v
	if tgt.get('pm_ra') is None or tgt.get('pm_decl') is None:
		pmtotal = undef
	else:
		pmtotal = np.sqrt(tgt['pm_ra']**2 + tgt['pm_decl']**2)
	hdr = header
	prim = [
		card('NEXTEND', 3 + int(has_weightmap), 'number of standard extensions'), card('EXTNAME', 'PRIMARY', 'name of extension'),
		card('ORIGIN', 'TASOC/Aarhus', 'institution responsible for creating this file'),
		card('DATE', datetime.datetime.now().strftime("%Y-%m-%d"), 'date the file was created'),
		card('TELESCOP', 'TESS', 'telescope'), card('INSTRUME', 'TESS Photometer', 'detector type'),
		card('FILTER', 'TESS', 'Photometric bandpass filter'), card('OBJECT', f"TIC {starid:d}", 'string version of TICID'),
		card('TICID', int(starid), 'unique TESS target identifier'), card('CAMERA', int(camera), 'Camera number'),
		card('CCD', int(ccd), 'CCD number'), card('SECTOR', int(sector), 'Observing sector'),
		card('PROCVER', PROCVER, 'Version of photometry pipeline'), card('FILEVER', '1.5', 'File format version'),
		card('DATA_REL', data_rel, 'Data release number'), card('VERSION', int(version), 'Version of the processing'),
		card('PHOTMET', method, 'Photometric method used'),
		card('RADESYS', 'ICRS', 'reference frame of celestial coordinates'), card('EQUINOX', 2000.0, 'equinox of celestial coordinate system'),
		card('RA_OBJ', tgt.get('ra_J2000'), '[deg] Right ascension'), card('DEC_OBJ', tgt.get('decl_J2000'), '[deg] Declination'),
		card('PMRA', opt('pm_ra'), '[mas/yr] RA proper motion'), card('PMDEC', opt('pm_decl'), '[mas/yr] Dec proper motion'),
		card('PMTOTAL', pmtotal, '[mas/yr] total proper motion'),
		card('TESSMAG', float(tgt['tmag']), '[mag] TESS magnitude'), card('TEFF', opt('teff'), '[K] Effective temperature'),
		card('TICVER', ticver, 'TESS Input Catalog version'),
		card('CRMITEN', hdr.get('CRMITEN'), 'spacecraft cosmic ray mitigation enabled'),
		card('CRBLKSZ', hdr.get('CRBLKSZ'), '[exposures] s/c cosmic ray mitigation block siz'),
		card('CRSPOC', hdr.get('CRSPOC'), 'SPOC cosmic ray cleaning enabled'),
	]
	for key, value in additional_headers.items(): # K2P2 settings, AP_CONT, ... (:1497-1499)
		if isinstance(value, (tuple, list)):
			prim.append(card(key, value[0], value[1] if len(value) > 1 else None))
		else:
			prim.append(card(key, value))
	prim.append(card('DATAVAL', 0, 'Data validation flags'))
	return prim


def table_columns():
	"""The 14 columns of the ``LIGHTCURVE`` table (:1507-1600) as :func:`fitsio.bintable_hdu` takes them, without their arrays: 96 bytes
	per row, ``D E J D D D D D J J D D D D`` -- the layout csrc/lctable_rules.h restates."""
	f64 = 'column format: 64-bit floating point'
	i32 = 'column format: signed 32-bit integer'
	disp = 'column display format'

	def column(name, fmt, unit=None, dsp=None, title=None, unitc=None):
		return {'name': name, 'format': fmt, 'unit': unit, 'disp': dsp,
			'comments': {'TTYPE': title, 'TFORM': f64 if fmt == 'D' else ('column format: 32-bit floating point' if fmt == 'E' else i32),
				'TUNIT': unitc, 'TDISP': disp}}
	return [
		column('TIME', 'D', 'BJD - 2457000, days', 'D14.7', 'column title: data time stamps', 'column units: Barycenter corrected TESS Julian'),
		column('TIMECORR', 'E', 'd', 'E13.6', 'column title: barycenter - timeslice correction', 'column units: day'),
		column('CADENCENO', 'J', None, 'I10', 'column title: unique cadence number'),
		column('FLUX_RAW', 'D', 'e-/s', 'E26.17', 'column title: photometric flux', 'column units: electrons per second'),
		column('FLUX_RAW_ERR', 'D', 'e-/s', 'E26.17', 'column title: photometric flux error', 'column units: electrons per second'),
		column('FLUX_BKG', 'D', 'e-/s', 'E26.17', 'column title: photometric background flux', 'column units: electrons per second'),
		column('FLUX_CORR', 'D', 'ppm', 'E26.17', 'column title: corrected photometric flux', 'column units: rel. flux in parts-per-million'),
		column('FLUX_CORR_ERR', 'D', 'ppm', 'E26.17', 'column title: corrected photometric flux error', 'column units: parts-per-million'),
		column('QUALITY', 'J', None, 'B16.16', 'column title: photometry quality flags'),
		column('PIXEL_QUALITY', 'J', None, 'B16.16', 'column title: pixel quality flags'),
		column('MOM_CENTR1', 'D', 'pixels', 'F10.5', 'column title: moment-derived column centroid', 'column units: pixels'),
		column('MOM_CENTR2', 'D', 'pixels', 'F10.5', 'column title: moment-derived row centroid', 'column units: pixels'),
		column('POS_CORR1', 'D', 'pixels', 'F14.7', 'column title: column position correction', 'column units: pixels'),
		column('POS_CORR2', 'D', 'pixels', 'F14.7', 'column title: row position correction', 'column units: pixels'),
	]


def _time_cards(time, cadence, hdr, num_frm, n_readout):
	"""The cards of the ``LIGHTCURVE`` header before the columns' (:1602-1641) from the kept ``time`` values."""
	cadence = int(cadence)
	n = len(time)
	# time keywords (:1602-1641)
	tdel = cadence / 86400
	tstart = float(time[0] - tdel/2) if n else float('nan')
	tstop = float(time[-1] + tdel/2) if n else float('nan')
	telapse = tstop - tstart
	frametime, int_time, readtime = 2.0, 1.98, 0.02
	if hdr.get('CRMITEN'):
		crblocksize = hdr['CRBLKSZ']
		deadc = (int_time * (crblocksize-2)/crblocksize) / frametime
	else:
		deadc = int_time / frametime
	bjdref = 2457000
	return [
		card('INHERIT', True, 'inherit the primary header'),
		card('TIMEREF', 'SOLARSYSTEM', 'barycentric correction applied to times'),
		card('TIMESYS', 'TDB', 'time system is Barycentric Dynamical Time (TDB)'),
		card('BJDREFI', bjdref, 'integer part of BTJD reference date'), card('BJDREFF', 0.0, 'fraction of the day in BTJD reference date'),
		card('TIMEUNIT', 'd', 'time unit for TIME, TSTART and TSTOP'),
		card('TSTART', tstart, 'observation start time in BTJD'), card('TSTOP', tstop, 'observation stop time in BTJD'),
		card('DATE-OBS', fitsio.tdb_to_utc_isot(tstart, bjdref) if n else None, 'TSTART as UTC calendar date'),
		card('DATE-END', fitsio.tdb_to_utc_isot(tstop, bjdref) if n else None, 'TSTOP as UTC calendar date'),
		card('MJD-BEG', tstart + (bjdref - 2400000.5), 'observation start time in MJD'),
		card('MJD-END', tstop + (bjdref - 2400000.5), 'observation start time in MJD'),
		card('TELAPSE', telapse, '[d] TSTOP - TSTART'), card('LIVETIME', telapse*deadc, '[d] TELAPSE multiplied by DEADC'),
		card('DEADC', deadc, 'deadtime correction'), card('EXPOSURE', telapse*deadc, '[d] time on source'),
		card('XPOSURE', frametime*deadc*num_frm, '[s] Duration of exposure'),
		card('TIMEPIXR', 0.5, 'bin time beginning=0 middle=0.5 end=1'), card('TIMEDEL', tdel, '[d] time resolution of data'),
		card('INT_TIME', int_time, '[s] photon accumulation time per frame'), card('READTIME', readtime, '[s] readout time per frame'),
		card('FRAMETIM', frametime, '[s] frame time (INT_TIME + READTIME)'), card('NUM_FRM', num_frm, 'number of frames per time stamp'),
		card('NREADOUT', int(n_readout), 'number of read per cadence'),
	]


#--------------------------------------------------------------------------------------------------
class FileInfo(object):
	"""
	What the light-curve files of a batch carry that the batched entry's arguments do not: ``sector, camera, ccd``, ``cadence``
	(seconds), ``n_readout``, ``num_frm`` (``NUM_FRM``; default: the header's, else 900, the reference's FFI value,
	BasePhotometry.py:269), ``header`` (the input file's: ``DATA_REL``, the cosmic-ray mitigation keywords), ``ticver``, ``wcs_header``
	(a callable ``stamp -> cards`` as ``source.wcs_header``; without one the stamp limits are written) and
	``backgrounds_pixels_used`` (default: the stack's).
	"""

	def __init__(self, sector, camera, ccd, cadence=1800, n_readout=720, num_frm=None, header=None, ticver=None, wcs_header=None, backgrounds_pixels_used=None):
		self.sector, self.camera, self.ccd = sector, camera, ccd
		self.cadence = int(cadence) if cadence else 1800
		self.n_readout = n_readout
		self.header = dict(header or {})
		self.data_rel = self.header.get('DATA_REL')
		self.num_frm = self.header.get('NUM_FRM', num_frm or 900)
		self.ticver = ticver
		self.wcs_header = wcs_header
		self.backgrounds_pixels_used = None if backgrounds_pixels_used is None else np.asarray(backgrounds_pixels_used, dtype=bool)

	@classmethod
	def from_source(cls, src):
		"""From a ``StampSource``: the attributes ``BasePhotometry.__init__`` reads from it for an ``ffi`` run."""
		return cls(src.sector, src.camera, src.ccd, cadence=src.cadence, n_readout=src.n_readout, num_frm=getattr(src, 'num_frm', None),
			header=getattr(src, 'header', None), ticver=getattr(src, 'ticver', None), wcs_header=getattr(src, 'wcs_header', None),
			backgrounds_pixels_used=getattr(src, 'backgrounds_pixels_used', None))


#: the optional catalogue columns of ``targets`` that go into the primary header (BasePhotometry.py:416-438)
_CATALOGUE_COLUMNS = ('ra_J2000', 'decl_J2000', 'pm_ra', 'pm_decl', 'teff')


def _crop(image, stamp, row0, col0):
	return image[stamp[0] - row0:stamp[1] - row0, stamp[2] - col0:stamp[3] - col0]


def save_lightcurves(results, stack, output_folder, info, time, quality, version, timecorr=None, cadenceno=None, targets=None, workers=None,
	compresslevel=9, timings=None, compress='zlib', table='host'):
	"""
	Write the light-curve file of every target of ``results`` (a ``tessphot.BatchResults`` over ``stack``) whose final status is OK
	or WARNING -- the rule of ``run_plugin`` (tessphot.py:52-53) --, as the per-target run would: same name, same folder,
	``_details['filepath_lightcurve']``.  Returns the list of paths (``None`` where no file was written), also kept as
	``results.filepaths``.  See ``BatchResults.save_lightcurves`` for the arguments; ``timings``: a dict that receives the seconds
	spent in ``quality`` (launch + download), ``build`` (bytes of the HDUs, summed over the workers) and ``gzip`` (likewise).
	``compress``: ``'zlib'`` (the default: gzip at ``compresslevel`` on the workers, the bytes ``gzip.open`` writes) or ``'device'``: the
	workers build the bytes, the calling thread compresses them on the stack's device (``deflate.gzip_many``) and the workers write the
	members -- the same content in other compressed bytes, which depend on the content alone; ``compresslevel`` is ignored, and
	``timings['gzip']`` is the wall time of the device path (``timings['write']``: writing the files, summed over the workers).
	``table``: ``'host'`` (the default) or, with ``compress='device'`` only, ``'device'``: the workers build the headers and the image
	HDUs, and per window the calling thread uploads the light curves, ``QUALITY`` rows and ``pos_corr``, writes the ``LIGHTCURVE`` data
	units with their DATASUMs on the device in one launch (``tp_lc_table_pack``: ``time`` is shared, so are the kept rows), places the
	host pieces around them and compresses from that buffer -- the same file bytes as ``compress='device'`` alone.  ``timings['table']``:
	the wall time of upload, pack and the download of the sums; ``timings['build']`` is then the host pieces only.
	"""
	import time as _clock
	if compress not in COMPRESS:
		raise ValueError(f"compress must be one of {COMPRESS}, not {compress!r}")
	_check_table(table, compress)
	if version is None:
		raise ValueError("VERSION has not been set")
	if targets is None:
		raise ValueError("the targets of the batch are needed for the files' primary headers")
	n = len(results)
	T = stack.n_cad
	time = np.asarray(time, dtype='float64')
	shared = {'time': time, 'timecorr': np.zeros(T) if timecorr is None else np.asarray(timecorr, dtype='float64'),
		'cadenceno': np.arange(T, dtype='int32') if cadenceno is None else np.asarray(cadenceno, dtype='int32'), 'quality': np.asarray(quality, dtype='int32')}
	if any(len(v) != T for v in shared.values()):
		raise ValueError("time, timecorr, cadenceno and quality must have one entry per frame of the stack")
	output_folder = os.path.abspath(output_folder)
	os.makedirs(output_folder, exist_ok=True)
	status = np.asarray(results.status)
	stamps = np.asarray(results.stamp, dtype='int64').reshape(n, 4)
	wanted = np.flatnonzero((status == STATUS.OK.value) | (status == STATUS.WARNING.value))

	# QUALITY of the whole batch: one launch over the final stamps (targets without a file: no stamp), one download of (N, T) int32
	t0 = _clock.perf_counter()
	final = np.full((n, 4), -1, dtype='int64')
	final[wanted] = stamps[wanted]
	flag_series = stack.stamp_flag_series(final, PIXEL_BACKGROUND_SHENANIGANS, CORRECTOR_BACKGROUND_SHENANIGANS)
	if timings is not None:
		timings['quality'] = timings.get('quality', 0.0) + _clock.perf_counter() - t0
	bpu = info.backgrounds_pixels_used if info.backgrounds_pixels_used is not None else stack.backgrounds_pixels_used
	region_sum = None
	if results.halo_rows:
		region_sum = stack.sumimage_for(shared['quality']).to_host()      # the Halo stamps' sum images are crops of the region's
	zeros2 = np.zeros((T, 2))
	from .plugins import K2P2_HEADERS, K2P2_SETTINGS      # (the cards AperturePhotometry.do_photometry sets; plugins imports this module)
	k2p2_headers = {key: (bool(K2P2_SETTINGS[name]) if isinstance(K2P2_SETTINGS[name], bool) else K2P2_SETTINGS[name], comment) for key, name, comment in K2P2_HEADERS}
	spent ={'build': 0.0, 'gzip': 0.0}

	def one(i):
		# (BatchResult of target i: built here, on the worker -- its arrays are views of the batch's block)
		r = results[i]
		stamp = tuple(int(v) for v in stamps[i])
		if r.method == 'halo':
			sumimage = _crop(region_sum, stamp, stack.row0, stack.col0)
			headers = dict(results.halo.headers)
		else:
			sumimage = results.frames[i]['sumimage']
			headers = dict(k2p2_headers)
			if 'contamination' in r._details:
				headers['AP_CONT'] = (r._details['contamination'], 'AP contamination')
		lc = dict(shared)
		for k in ('flux', 'flux_err', 'flux_background', 'pos_centroid'):
			lc[k] = r.lightcurve[k]
		lc['pos_corr'] = results.pos_corr[i] if results.pos_corr is not None else zeros2
		target = {'tmag': targets['tmag'][i]}
		for k in _CATALOGUE_COLUMNS:
			if k in targets:
				target[k] = targets[k][i]
		# (the aperture plugin positions on its photometry mask; the Halo plugin has no position mask)
		aperture = aperture_with_masks(ffi_aperture(sumimage, stamp, bpu, stack.row0, stack.col0), r.final_phot_mask, None if r.method == 'halo' else r.final_phot_mask)
		ta = _clock.perf_counter()
		args = (target, int(results.starid[i]), info.sector, info.camera, info.ccd, info.cadence, info.data_rel, version, r.method, info.ticver,
			info.header, info.num_frm, info.n_readout, headers)
		path = os.path.join(output_folder, lightcurve_filename(results.starid[i], info.sector, info.camera, info.ccd, info.cadence, info.data_rel, version))
		if table == 'device':
			pieces = lightcurve_pieces(*args, time, sumimage, aperture, image_cards(stamp, info.wcs_header), weightmap=r.halo_weightmap)
			spent_here = _clock.perf_counter() - ta
			centroid = np.asarray(lc['pos_centroid'])
			source = {'time': time, 'lc': (lc['flux'], lc['flux_err'], lc['flux_background'], centroid[:, 0], centroid[:, 1]), 'quality': flag_series[i],
				'pos_corr': results.pos_corr[i] if results.pos_corr is not None else None}
			return path, pieces, source, spent_here
		hdus = lightcurve_hdus(*args, lc, flag_series[i], sumimage, aperture, image_cards(stamp, info.wcs_header), weightmap=r.halo_weightmap)
		return path, hdus, _clock.perf_counter() - ta

	paths = [None] * n
	vectors = {'time': time, 'timecorr': shared['timecorr'], 'cadenceno': shared['cadenceno'], 'pixel_quality': shared['quality']}   # (table='device': stride 0)
	for i, path in zip(wanted, _write_files(one, wanted, workers, compress, compresslevel, getattr(stack, 'ctx', None), spent, table=table, shared=vectors)):
		paths[int(i)] = path
	if timings is not None:
		_add_timings(timings, spent)
	results.filepaths = paths
	results._filepath_rel = {int(i): relative_filepath(paths[int(i)], output_folder, output_folder) for i in wanted}
	return paths


def save_tpf_lightcurves(results, output_folder, version, workers=None, compresslevel=9, timings=None, compress='zlib', ctx=None, table='host'):
	"""
	The light-curve files of a ``tessphot.TpfBatchResults`` (a chunk of ``tessphot_tpfs``): for every target whose final status is OK or
	WARNING the file ``tessphot('aperture', starid, TpfStampSource(...), output_folder, datasource='tpf')`` writes.  Every file has a
	:class:`FileInfo` of its own, from its headers as :meth:`FileInfo.from_source` takes it from the ``TpfStampSource``; ``TIME`` ..
	``PIXEL_QUALITY`` and ``POS_CORR1/2`` are the file's columns, ``QUALITY`` is all zero (a target pixel file brings no pixel flags),
	the ``APERTURE`` image is the file's without SPOC's mask and centroid flags plus this run's, the image cards are the stamp's
	limits.  A target done with Halo photometry (``tessphot_tpfs(method=None)`` or ``'halo'``) gets the file of the per-file Halo run: the
	``HALO_*`` cards in place of the K2P2 ones, the Halo mask without a position mask and the ``WEIGHTMAP`` extension; a target done with
	LinPSF photometry (``method='linpsf'``) the file of the per-file LinPSF run: ``PSF_FERR`` / ``PSF_CONT`` and no mask bits.  Threads, ``compresslevel``, ``timings`` (``build`` / ``gzip``), ``compress`` and the return value as :func:`save_lightcurves`;
	``compress='device'`` runs on ``ctx`` (default: the context the results were computed on), whose owner the calling thread must be.
	``table='device'`` (with ``compress='device'``) as in :func:`save_lightcurves`; here every file has its own ``time`` .. ``PIXEL_QUALITY``,
	so the vectors are strided per target and there is one ``tp_lc_table_pack`` per set of files with one length and one list of kept rows.
	"""
	import time as _clock
	if compress not in COMPRESS:
		raise ValueError(f"compress must be one of {COMPRESS}, not {compress!r}")
	_check_table(table, compress)
	ctx = getattr(results, 'ctx', None) if ctx is None else ctx
	if compress == 'device' and ctx is None:
		raise ValueError("compress='device' needs the context of the batch (ctx=)")
	if version is None:
		raise ValueError("VERSION has not been set")
	n = len(results)
	output_folder = os.path.abspath(output_folder)
	os.makedirs(output_folder, exist_ok=True)
	status = np.asarray(results.status)
	wanted = np.flatnonzero((status == STATUS.OK.value) | (status == STATUS.WARNING.value))
	from .plugins import K2P2_HEADERS, K2P2_SETTINGS
	k2p2_headers = {key: (bool(K2P2_SETTINGS[name]) if isinstance(K2P2_SETTINGS[name], bool) else K2P2_SETTINGS[name], comment) for key, name, comment in K2P2_HEADERS}

	def one(i):
		r = results[i]
		ld = results.loaded[i]
		header = dict(ld.header)
		header['TIME_OFFSET_CORRECTED'] = bool(ld.time_offset_corrected)
		info = FileInfo(ld.sector, ld.camera, ld.ccd, cadence=ld.cadence, n_readout=ld.n_readout, num_frm=ld.num_frm or 60, header=header)   # (60: BasePhotometry.py:372)
		if r.method == 'halo':
			headers = dict(results.halo.headers)
		elif r.method == 'linpsf':
			headers = dict(r.additional_headers)                             # (PSF_FERR, PSF_CONT: no mask was made, no K2P2 cards)
		else:
			headers = dict(k2p2_headers)
			if 'contamination' in r._details:
				headers['AP_CONT'] = (r._details['contamination'], 'AP contamination')
		stamp = tuple(int(v) for v in ld.max_stamp)
		T = len(r.lightcurve['time'])
		# (the aperture plugin positions on its photometry mask; the Halo plugin has no position mask)
		aperture = aperture_with_masks(results.aperture_image(i), r.final_phot_mask, None if r.method == 'halo' else r.final_phot_mask)
		ta = _clock.perf_counter()
		args = ({'tmag': float(results.tmag[i])}, int(results.starid[i]), info.sector, info.camera, info.ccd, info.cadence, info.data_rel, version, r.method,
			info.ticver, info.header, info.num_frm, info.n_readout, headers)
		path = os.path.join(output_folder, lightcurve_filename(results.starid[i], info.sector, info.camera, info.ccd, info.cadence, info.data_rel, version))
		if table == 'device':
			lc = r.lightcurve
			pieces = lightcurve_pieces(*args, lc['time'], results.sumimage(i), aperture, image_cards(stamp), weightmap=r.halo_weightmap)
			spent_here = _clock.perf_counter() - ta
			centroid = np.asarray(lc['pos_centroid'])
			source = {'time': lc['time'], 'timecorr': lc['timecorr'], 'cadenceno': lc['cadenceno'], 'pixel_quality': lc['quality'],
				'lc': (lc['flux'], lc['flux_err'], lc['flux_background'], centroid[:, 0], centroid[:, 1]), 'quality': None, 'pos_corr': lc['pos_corr']}
			return path, pieces, source, spent_here
		hdus = lightcurve_hdus(*args, r.lightcurve, np.zeros(T, dtype='int32'), results.sumimage(i), aperture, image_cards(stamp), weightmap=r.halo_weightmap)
		return path, hdus, _clock.perf_counter() - ta

	spent = {'build': 0.0, 'gzip': 0.0}
	paths = [None] * n
	for i, path in zip(wanted, _write_files(one, wanted, workers, compress, compresslevel, ctx, spent, table=table)):
		paths[int(i)] = path
	if timings is not None:
		_add_timings(timings, spent)
	results.filepaths = paths
	results._filepath_rel = {int(i): relative_filepath(paths[int(i)], output_folder, output_folder) for i in wanted}
	return paths
