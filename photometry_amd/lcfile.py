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
"""

import datetime
import os
from concurrent.futures import ThreadPoolExecutor
import numpy as np
from . import fitsio
from .fitsio import card
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
#: files whose bytes are held at a time with ``compress='device'``: built, compressed in batches, written, then the next window
DEVICE_WINDOW = 256


def _add_timings(timings, spent):
	for k, v in spent.items():
		if isinstance(v, dict):
			_add_timings(timings.setdefault(k, {}), v)
		else:
			timings[k] = timings.get(k, 0.0) + v


def _write_files(build, wanted, workers, compress, compresslevel, ctx, spent):
	"""
	The files of the targets ``wanted``: ``build(i) -> (path, hdus, seconds)`` on ``workers`` threads, then the gzip member.
	``'zlib'``: the worker that built the bytes compresses and writes them (``fitsio.write``).  ``'device'``: per window of
	:data:`DEVICE_WINDOW` files the workers build the bytes, the calling thread -- the owner of ``ctx`` -- compresses them in batches
	(``deflate.gzip_many``), and the workers write the members.  Returns the paths in the order of ``wanted``; adds the seconds to
	``spent['build']`` and ``spent['gzip']`` (``'device'``: the wall time of the device path, its parts as ``deflate.gzip_many`` names
	them in ``spent['gzip_parts']``, and ``spent['write']`` for the files).
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
			built = run(build_one, wanted[a:a + DEVICE_WINDOW])
			spent['build'] += sum(b[2] for b in built)
			tb = _clock.perf_counter()
			members = deflate.gzip_many(ctx, [b[1] for b in built], parts=spent.setdefault('gzip_parts', {}))
			spent['gzip'] += _clock.perf_counter() - tb
			spent['write'] = spent.get('write', 0.0) + sum(run(write_one, [(b[0], m) for b, m in zip(built, members)]))
			paths.extend(b[0] for b in built)
	finally:
		if pool is not None:
			pool.shutdown()
	return paths


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
	cadence = int(cadence)
	SumImage = np.asarray(sumimage, dtype='float64')
	indx = np.isfinite(np.asarray(lightcurve['time']))
	quality = np.asarray(quality)[indx]
	col = {k: np.asarray(lightcurve[k])[indx] for k in lightcurve.keys()}
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
		card('NEXTEND', 3 + int(weightmap is not None), 'number of standard extensions'), card('EXTNAME', 'PRIMARY', 'name of extension'),
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

	n = len(col['time'])
	nan = np.full(n, np.nan)
	f64 = 'column format: 64-bit floating point'
	i32 = 'column format: signed 32-bit integer'
	disp = 'column display format'

	def column(name, fmt, arr, unit=None, dsp=None, title=None, unitc=None):
		return {'name': name, 'format': fmt, 'array': arr, 'unit': unit, 'disp': dsp,
			'comments': {'TTYPE': title, 'TFORM': f64 if fmt == 'D' else ('column format: 32-bit floating point' if fmt == 'E' else i32),
				'TUNIT': unitc, 'TDISP': disp}}
	columns = [
		column('TIME', 'D', col['time'], 'BJD - 2457000, days', 'D14.7', 'column title: data time stamps', 'column units: Barycenter corrected TESS Julian'),
		column('TIMECORR', 'E', col['timecorr'], 'd', 'E13.6', 'column title: barycenter - timeslice correction', 'column units: day'),
		column('CADENCENO', 'J', col['cadenceno'], None, 'I10', 'column title: unique cadence number'),
		column('FLUX_RAW', 'D', col['flux'], 'e-/s', 'E26.17', 'column title: photometric flux', 'column units: electrons per second'),
		column('FLUX_RAW_ERR', 'D', col['flux_err'], 'e-/s', 'E26.17', 'column title: photometric flux error', 'column units: electrons per second'),
		column('FLUX_BKG', 'D', col['flux_background'], 'e-/s', 'E26.17', 'column title: photometric background flux', 'column units: electrons per second'),
		column('FLUX_CORR', 'D', nan, 'ppm', 'E26.17', 'column title: corrected photometric flux', 'column units: rel. flux in parts-per-million'),
		column('FLUX_CORR_ERR', 'D', nan, 'ppm', 'E26.17', 'column title: corrected photometric flux error', 'column units: parts-per-million'),
		column('QUALITY', 'J', quality, None, 'B16.16', 'column title: photometry quality flags'),
		column('PIXEL_QUALITY', 'J', col['quality'], None, 'B16.16', 'column title: pixel quality flags'),
		column('MOM_CENTR1', 'D', col['pos_centroid'][:, 0], 'pixels', 'F10.5', 'column title: moment-derived column centroid', 'column units: pixels'),
		column('MOM_CENTR2', 'D', col['pos_centroid'][:, 1], 'pixels', 'F10.5', 'column title: moment-derived row centroid', 'column units: pixels'),
		column('POS_CORR1', 'D', col['pos_corr'][:, 0], 'pixels', 'F14.7', 'column title: column position correction', 'column units: pixels'),
		column('POS_CORR2', 'D', col['pos_corr'][:, 1], 'pixels', 'F14.7', 'column title: row position correction', 'column units: pixels'),
	]
	# time keywords (:1602-1641)
	tdel = cadence / 86400
	tstart = float(col['time'][0] - tdel/2) if n else float('nan')
	tstop = float(col['time'][-1] + tdel/2) if n else float('nan')
	telapse = tstop - tstart
	frametime, int_time, readtime = 2.0, 1.98, 0.02
	if hdr.get('CRMITEN'):
		crblocksize = hdr['CRBLKSZ']
		deadc = (int_time * (crblocksize-2)/crblocksize) / frametime
	else:
		deadc = int_time / frametime
	bjdref = 2457000
	tcards = [
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
	# image extensions: the cards of the stamp, then INHERIT
	icards = list(image_cards) + [card('INHERIT', True, 'inherit the primary header')]
	hdus = [fitsio.primary_hdu(prim), fitsio.bintable_hdu('LIGHTCURVE', columns, tcards),
		fitsio.image_hdu('SUMIMAGE', SumImage, icards), fitsio.image_hdu('APERTURE', np.asarray(aperture, dtype='int32'), icards)]
	if weightmap is not None:
		hdus.append(weightmap_hdu(weightmap, SumImage.shape, icards))
	return hdus


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
	compresslevel=9, timings=None, compress='zlib'):
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
	"""
	import time as _clock
	if compress not in COMPRESS:
		raise ValueError(f"compress must be one of {COMPRESS}, not {compress!r}")
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
		hdus = lightcurve_hdus(target, int(results.starid[i]), info.sector, info.camera, info.ccd, info.cadence, info.data_rel, version, r.method, info.ticver,
			info.header, info.num_frm, info.n_readout, headers, lc, flag_series[i], sumimage, aperture, image_cards(stamp, info.wcs_header), weightmap=r.halo_weightmap)
		path = os.path.join(output_folder, lightcurve_filename(results.starid[i], info.sector, info.camera, info.ccd, info.cadence, info.data_rel, version))
		return path, hdus, _clock.perf_counter() - ta

	paths = [None] * n
	for i, path in zip(wanted, _write_files(one, wanted, workers, compress, compresslevel, getattr(stack, 'ctx', None), spent)):
		paths[int(i)] = path
	if timings is not None:
		_add_timings(timings, spent)
	results.filepaths = paths
	results._filepath_rel = {int(i): relative_filepath(paths[int(i)], output_folder, output_folder) for i in wanted}
	return paths


def save_tpf_lightcurves(results, output_folder, version, workers=None, compresslevel=9, timings=None, compress='zlib', ctx=None):
	"""
	The light-curve files of a ``tessphot.TpfBatchResults`` (a chunk of ``tessphot_tpfs``): for every target whose final status is OK or
	WARNING the file ``tessphot('aperture', starid, TpfStampSource(...), output_folder, datasource='tpf')`` writes.  Every file has a
	:class:`FileInfo` of its own, from its headers as :meth:`FileInfo.from_source` takes it from the ``TpfStampSource``; ``TIME`` ..
	``PIXEL_QUALITY`` and ``POS_CORR1/2`` are the file's columns, ``QUALITY`` is all zero (a target pixel file brings no pixel flags),
	the ``APERTURE`` image is the file's without SPOC's mask and centroid flags plus this run's, the image cards are the stamp's
	limits.  Threads, ``compresslevel``, ``timings`` (``build`` / ``gzip``), ``compress`` and the return value as :func:`save_lightcurves`;
	``compress='device'`` runs on ``ctx`` (default: the context the results were computed on), whose owner the calling thread must be.
	"""
	import time as _clock
	if compress not in COMPRESS:
		raise ValueError(f"compress must be one of {COMPRESS}, not {compress!r}")
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
		headers = dict(k2p2_headers)
		if 'contamination' in r._details:
			headers['AP_CONT'] = (r._details['contamination'], 'AP contamination')
		stamp = tuple(int(v) for v in ld.max_stamp)
		T = len(r.lightcurve['time'])
		aperture = aperture_with_masks(results.aperture_image(i), r.final_phot_mask, r.final_phot_mask)
		ta = _clock.perf_counter()
		hdus = lightcurve_hdus({'tmag': float(results.tmag[i])}, int(results.starid[i]), info.sector, info.camera, info.ccd, info.cadence, info.data_rel, version, r.method,
			info.ticver, info.header, info.num_frm, info.n_readout, headers, r.lightcurve, np.zeros(T, dtype='int32'), results.sumimage(i), aperture, image_cards(stamp))
		path = os.path.join(output_folder, lightcurve_filename(results.starid[i], info.sector, info.camera, info.ccd, info.cadence, info.data_rel, version))
		return path, hdus, _clock.perf_counter() - ta

	spent = {'build': 0.0, 'gzip': 0.0}
	paths = [None] * n
	for i, path in zip(wanted, _write_files(one, wanted, workers, compress, compresslevel, ctx, spent)):
		paths[int(i)] = path
	if timings is not None:
		_add_timings(timings, spent)
	results.filepaths = paths
	results._filepath_rel = {int(i): relative_filepath(paths[int(i)], output_folder, output_folder) for i in wanted}
	return paths
