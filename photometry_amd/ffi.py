# -*- coding: utf-8 -*-
"""
Calibrated full-frame images (``*_ffic.fits``) into device-resident frame stacks: the input side of the prepare stage.

The reference opens every file with astropy (``io.FFIImage``, io.py:25-93): the science region ``[0:2048, 44:2092]`` of the image
HDU and of the uncertainty HDU as native float32, the primary header merged with the image header, and a handful of cards the
prepare stage reads per file (prepare.py:375-405).  Here the header blocks are parsed on the host (``fitsio.read_header_blocks``;
the CPU copies the data units but never converts them), the bytes of the two data units travel over the link exactly as they lie in the file,
and the byte swap, the crop and the placement into frame ``k`` of the ``(T, R, C)`` stacks happen in HBM (``tp_fits_unpack``,
csrc/fitsin.hip).  The FITS ``DATASUM`` of every unit is checked on the device as well (``tp_fits_datasum``).

:func:`find_ffi_files` is the reference's file-name rule, :func:`read_ffi_header` what ``FFIImage`` learns from the headers,
:func:`load_ffis` the streaming loader and :func:`prepare_ffis` the prepare stage from a list of files to a ``.tpstack``.

Not covered: integer images (``BSCALE`` / ``BZERO``), tile-compressed FITS, the smear rows, and the time-offset fix of early data
releases for FFIs (``fixes.time_offset``: the adapter's job, see plugins.py; ``tpf.time_offset`` restates the rule for both data
types).  Target pixel files have a loader of their own, ``photometry_amd.tpf``.
"""

import logging
import os
import re
import time as _time
from collections import namedtuple
import numpy as np
from . import fitsio
from . import wcs as wcsmod
from .device import round_up
from .staging import StagedUpload, check_datasum

#: the science region of a TESS FFI (io.py:47-48) and the shape that marks one (io.py:46)
TESS_SHAPE = (2078, 2136)
TESS_WINDOW = (0, 44, 2048, 2048)   # row0, col0, rows, cols
#: cards that have to be the same in every file of a CCD (prepare.py:362-372)
ATTRIBUTES = ('CAMERA', 'CCD', 'DATA_REL', 'PROCVER', 'NUM_FRM', 'NREADOUT', 'CRMITEN', 'CRBLKSZ', 'CRSPOC')
#: smoothing widths prepare_frames knows (prepare.py:258)
CADENCES = (1800, 600)

# the keywords of the primary WCS description (alternate descriptions carry a letter: CTYPE1P, ...), and the image size
# calc_footprint reads
_WCS_KEY = re.compile(r"^(WCSAXES|CTYPE\d|CUNIT\d|CRPIX\d|CRVAL\d|CDELT\d|CROTA\d|CD\d_\d|PC\d_\d|PV\d_\d+|PS\d_\d+|LONPOLE|LATPOLE|RADESYS|EQUINOX|"
	r"A_ORDER|B_ORDER|AP_ORDER|BP_ORDER|A_\d_\d|B_\d_\d|AP_\d_\d|BP_\d_\d|A_DMAX|B_DMAX|CPDIS\d|CQDIS\d|D2IMDIS\d|NAXIS1|NAXIS2)$")

#: where a data unit lies in its file: HDU number, byte offset, BITPIX, (NAXIS2, NAXIS1), bytes with the padding, the DATASUM card (or None)
DataUnit = namedtuple('DataUnit', 'hdu offset bitpix shape nbytes datasum')
FFIHeader = namedtuple('FFIHeader', 'path header is_tess image uncert wcs_cards')


class ChecksumError(ValueError):
	"""A data unit does not add up to its ``DATASUM`` card."""


class LoadedFFIs(object):
	"""What :func:`load_ffis` returns (see there); ``free()`` releases the two stacks."""

	def free(self):
		for name in ('raw', 'raw_err'):
			a = self.__dict__.get(name)
			if a is not None:
				a.free()
			self.__dict__[name] = None


#--------------------------------------------------------------------------------------------------
def find_ffi_files(rootdir, sector=None, camera=None, ccd=None):
	"""
	Full paths of the calibrated FFIs below ``rootdir`` (searched recursively, links followed), optionally of one sector, camera
	or CCD, sorted by file name, i.e. by time: the file-name rule of io.py:123-166 (``tess<time>-s<sector>-<camera>-<ccd>-<4
	digits>-<x|s|a|b>_ffic.fits``, optionally ``.gz``).  Not cached: a second call sees what has changed on disk.
	"""
	sector_str = r'\d{4}' if sector is None else f'{int(sector):04d}'
	camera = r'\d' if camera is None else str(int(camera))
	ccd = r'\d' if ccd is None else str(int(ccd))
	regexp = re.compile(r'^tess\d+-s(?P<sector>' + sector_str + ')-(?P<camera>' + camera + r')-(?P<ccd>' + ccd + r')-\d{4}-[xsab]_ffic\.fits(\.gz)?$')
	matches = []
	for root, _, filenames in os.walk(rootdir, followlinks=True):
		for filename in filenames:
			if regexp.match(filename):
				matches.append(os.path.join(root, filename))
	matches.sort(key=os.path.basename)
	return matches


def _sector_of(path):
	m = re.match(r'^tess\d+-s(\d{4})-\d-\d-\d{4}-[xsab]_ffic\.fits(\.gz)?$', os.path.basename(str(path)))
	return int(m.group(1)) if m else None


def sector_cadence(sector):
	"""The FFI cadence in seconds of a TESS sector, as the reference's sector table gives it (``io.load_sector_settings``):
	1800 up to sector 26, 600 up to sector 54, 200 from sector 55."""
	sector = int(sector)
	return 1800 if sector <= 26 else 600 if sector <= 54 else 200


#--------------------------------------------------------------------------------------------------
def extrapolate_ffiindex(tstart, tstop, barycorr=0.0):
	"""The cadence number of an FFI without ``FFIINDEX`` card (before sector 6) from its timestamps (io.py:56-67): a straight line
	through cadence 4697 with 1800 s per cadence."""
	time = 0.5 * (tstart + tstop)
	first_time = 0.5 * (1325.317007851970 + 1325.337841177751) - 3.9072474e-03
	first_cadenceno = 4697
	timedelt = 1800 / 86400
	offset = first_cadenceno - first_time / timedelt
	return int(np.round((time - barycorr) / timedelt + offset))


def read_ffi_header(path):
	"""
	What ``FFIImage`` learns from the headers of an FFI, reading header blocks only (the data units are skipped with ``seek``, so a
	file cut short behind its last header still answers).  Returns an :class:`FFIHeader`:

	``header``: the primary header, for a TESS file updated by that of the first extension (io.py:51-52) and, when ``FFIINDEX`` is
	missing and ``EXPOSURE * 86400 > 1000``, with the extrapolated ``FFIINDEX`` (io.py:56-67).
	``is_tess``: ``TELESCOP == 'TESS'`` in the primary header and a first extension of 2136 x 2078 (io.py:46).
	``image`` / ``uncert``: the :class:`DataUnit` of image and uncertainty -- HDU 1 and 2 of a TESS file, else HDU 0 and 1 (io.py:80-82).
	``wcs_cards``: the raw 80-column cards of the HDU that holds the WCS, as one string: HDU 1 for every file (io.py:42).
	"""
	path = str(path)
	hdus = []
	for n, u in enumerate(fitsio.scan_hdus(path, 3)):
		datasum = u.header.get('DATASUM')
		hdus.append((u.header, u.cards, DataUnit(n, u.offset, u.header.get('BITPIX'), u.shape, u.nbytes, None if datasum is None else int(str(datasum).strip()))))
	if len(hdus) < 2:
		raise ValueError(f"{path}: an FFI has a primary HDU and at least one extension")
	hdr0, hdr1 = hdus[0][0], hdus[1][0]
	is_tess = hdr0.get('TELESCOP') == 'TESS' and hdr1.get('NAXIS1') == TESS_SHAPE[1] and hdr1.get('NAXIS2') == TESS_SHAPE[0]
	if is_tess:
		if len(hdus) < 3:
			raise ValueError(f"{path}: a TESS FFI has an image and an uncertainty extension")
		header = dict(hdr0)
		header.update(hdr1)
		if 'FFIINDEX' not in header and header['EXPOSURE'] * 86400 > 1000:
			header['FFIINDEX'] = extrapolate_ffiindex(header['TSTART'], header['TSTOP'], header.get('BARYCORR', 0))
		image, uncert = hdus[1][2], hdus[2][2]
	else:
		header = dict(hdr0)
		image, uncert = hdus[0][2], hdus[1][2]
	return FFIHeader(path, header, bool(is_tess), image, uncert, ''.join(hdus[1][1]))


def wcs_header_string(cards):
	"""The WCS keywords (and ``NAXIS1`` / ``NAXIS2``) of a string of 80-column cards, as a string of 80-column cards; '' without ``CTYPE1``."""
	keep = [cards[i:i + 80] for i in range(0, len(cards), 80) if cards[i + 8:i + 10] == '= ' and _WCS_KEY.match(cards[i:i + 8].strip())]
	if not any(c.startswith('CTYPE1 ') for c in keep):
		return ''
	return ''.join(c.ljust(80) for c in keep)


#--------------------------------------------------------------------------------------------------
def load_ffis(ctx, files, verify=True):
	"""
	Load the FFIs ``files`` (in the order given) into two float32 stacks on the device.  Returns a :class:`LoadedFFIs` with

	``raw``, ``raw_err``: float32 DeviceArrays ``(T, R, C)``: the science region of image and uncertainty of every file;
	``headers``: the dict ``prepare.prepare_frames`` takes (``is_tess``, ``CAMERA``, ``CCD``, ``FFIINDEX``, ``TSTART``, ``TSTOP``);
	``time`` (``0.5 * (TSTART + TSTOP)``), ``time_start``, ``time_stop``, ``timecorr`` (``BARYCORR``, default 0, float32),
	``quality`` (``DQUALITY``, default 0), ``cadenceno`` (``FFIINDEX``; without it ``RuntimeError`` for TESS data, else ``k + 1``):
	the vectors of prepare.py:393-405;
	``wcs_headers``: per frame the WCS keywords of its header as a string of 80-column cards ('' without any);
	``attributes``: the cards of :data:`ATTRIBUTES` from the first file (one that differs in a later file is logged as an error,
	prepare.py:382-388); ``row_offset``, ``col_offset``: 0 / 44 for TESS, else 0 / 0 (prepare.py:481-486); ``backapp``: the
	``BACKAPP`` card; ``files``; ``stats``: seconds the host spent reading and waiting.

	Every header is read and every file's geometry held to the first one's before anything is allocated (``ValueError`` naming the
	file).  The files then stream through two page-locked staging buffers on a second context (``staging.StagedUpload``): while
	file ``i`` transfers and unpacks, file ``i + 1`` is read (``readinto``; a ``.gz`` is decompressed) straight into the other
	buffer.  ``verify``: the word sum of every data unit that has a ``DATASUM`` card is formed on the device and compared once all
	files are in; a mismatch raises :class:`ChecksumError` naming file and HDU.  After any exception the staging buffers, events
	and both stacks are gone, the stacks only once nothing queued can write into them any more.
	"""
	logger = logging.getLogger(__name__)
	files = [str(f) for f in files]
	if not files:
		raise ValueError("load_ffis: no files")
	infos = [read_ffi_header(f) for f in files]
	first = infos[0]
	for h in infos:
		for unit in (h.image, h.uncert):
			if unit.bitpix not in (-32, -64) or len(unit.shape) != 2:
				raise ValueError(f"{h.path}: HDU {unit.hdu} is not a float image (BITPIX {unit.bitpix}, shape {unit.shape}); integer images are not supported")
		if h.image.shape != h.uncert.shape:
			raise ValueError(f"{h.path}: image {h.image.shape} and uncertainty {h.uncert.shape} differ in shape")
		if h.is_tess != first.is_tess or h.image.shape != first.image.shape:
			raise ValueError(f"{h.path}: shape {h.image.shape} (TESS: {h.is_tess}) differs from that of {first.path}: {first.image.shape} (TESS: {first.is_tess})")
	T = len(files)
	is_tess = first.is_tess
	row0, col0, R, C = TESS_WINDOW if is_tess else (0, 0) + first.image.shape

	# the vectors of prepare.py:393-405
	out = LoadedFFIs()
	hdrs = [h.header for h in infos]
	try:
		out.time_start = np.array([h['TSTART'] for h in hdrs], dtype='float64')
		out.time_stop = np.array([h['TSTOP'] for h in hdrs], dtype='float64')
	except KeyError as e:
		raise ValueError(f"load_ffis: a file lacks the {e.args[0]} card") from e
	out.time = 0.5 * (out.time_start + out.time_stop)
	out.timecorr = np.array([h.get('BARYCORR', 0) for h in hdrs], dtype='float32')
	out.quality = np.array([h.get('DQUALITY', 0) for h in hdrs], dtype='int32')
	out.cadenceno = np.empty(T, dtype='int32')
	for k, h in enumerate(hdrs):
		if 'FFIINDEX' in h:
			out.cadenceno[k] = h['FFIINDEX']
		elif is_tess:
			raise RuntimeError("Could not determine CADENCENO for TESS data")
		else:
			out.cadenceno[k] = k + 1
	out.attributes = {key: hdrs[0].get(key) for key in ATTRIBUTES}
	for k, h in enumerate(hdrs[1:], start=1):
		for key, value in out.attributes.items():
			if h.get(key) != value:
				logger.error("%04d: %s is not constant! (%s, %s)", k, key, value, h.get(key))
	out.backapp = bool(hdrs[0].get('BACKAPP', False))
	if any(bool(h.get('BACKAPP', False)) != out.backapp for h in hdrs):
		logger.error("BACKAPP is not constant! The first file's (%s) is used.", out.backapp)
	have_index = all('FFIINDEX' in h for h in hdrs)
	out.headers = {'is_tess': is_tess, 'CAMERA': hdrs[0].get('CAMERA'), 'CCD': hdrs[0].get('CCD'),
		'FFIINDEX': np.array([h['FFIINDEX'] for h in hdrs], dtype='int64') if have_index else None, 'TSTART': out.time_start, 'TSTOP': out.time_stop}
	out.wcs_headers = [wcs_header_string(h.wcs_cards) for h in infos]
	out.row_offset, out.col_offset = 0, col0
	out.is_tess = is_tess
	out.files = files
	out.raw = out.raw_err = None

	# from the first byte of the image unit to the last of the uncertainty unit: what is read from a file
	span = [(h.image.offset, h.uncert.offset + h.uncert.nbytes - h.image.offset) for h in infos]
	half = round_up(max(h.image.nbytes for h in infos), 256)            # every unit starts on a 256-byte boundary in device memory
	slot_bytes = half + round_up(max(h.uncert.nbytes for h in infos), 256)
	tic = _time.perf_counter()
	try:
		out.raw = ctx.empty((T, R, C), 'float32')
		out.raw_err = ctx.empty((T, R, C), 'float32')
		with StagedUpload(ctx, max(n for _, n in span), slot_bytes, 2 * T if verify else 0) as st:
			up = st.up
			for i, h in enumerate(infos):
				st.take()
				st.read(h.path, *span[i])
				units = ((h.image, out.raw, st.slot), (h.uncert, out.raw_err, st.slot + half))
				for unit, _, d_unit in units:
					st.upload(d_unit, unit.nbytes, unit.offset - span[i][0])
				st.record()
				for j, (unit, dst, d_unit) in enumerate(units):
					if verify and unit.datasum is not None:
						st.datasum(d_unit, unit.nbytes, 2 * i + j)
					up._check(up.lib.tp_fits_unpack(up.handle, d_unit, unit.bitpix, unit.shape[1], unit.shape[0], row0, col0, R, C, dst.ptr + i * R * C * 4, C))
			sums = st.finish()
		if verify:
			for i, h in enumerate(infos):
				for j, unit in enumerate((h.image, h.uncert)):
					check_datasum(h.path, unit.hdu, sums[2 * i + j], unit.datasum)
	except BaseException:
		out.free()                                                      # (the transfer context has been synced: nothing can write into the stacks any more)
		raise
	out.stats = dict(st.stats, bytes=int(sum(n for _, n in span)), total_s=_time.perf_counter() - tic)
	return out


#--------------------------------------------------------------------------------------------------
def check_wcs_headers(ctx, wcs_headers):
	"""
	prepare.py:433-447 for a list of header strings: a frame whose WCS does not bring its first footprint corner back through
	``all_world2pix`` (``wcs.footprint_check``: one launch for all frames), or whose keywords are outside TAN / TAN-SIP, gets the
	empty string.  Returns ``(strings, bad bool (T,))``; frames that had no WCS keywords count as bad.
	"""
	logger = logging.getLogger(__name__)
	strings = [str(h) for h in wcs_headers]
	parsed, index = [], []
	for k, h in enumerate(strings):
		if not h.strip():
			continue
		try:
			parsed.append(wcsmod.TanSipWCS.from_header(h))
			index.append(k)
		except ValueError as e:
			logger.info("%04d has bad WCS (%s).", k, e)
			strings[k] = ''
	if parsed:
		d_params = ctx.array(wcsmod.pack(parsed))
		status = wcsmod.footprint_check(ctx, d_params, len(parsed))
		for k, st in zip(index, status):
			if st != 0:
				logger.info("%04d has bad WCS.", k)
				strings[k] = ''
	return strings, np.array([not s.strip() for s in strings], dtype=bool)


def prepare_ffis(ctx, files_or_loaded, reference_time=None, cadence=None, calc_movement_kernel=False, write=None, verify=True, sector=None,
	flux_cutoff=8e4, backgrounds_pixels_threshold=0.5):
	"""
	The prepare stage from FFI files to prepared stacks: :func:`load_ffis` (unless a :class:`LoadedFFIs` is given),
	``prepare.prepare_frames`` with the loaded headers, and the bookkeeping of ``prepare_photometry`` around it:

	* the time vector has to rise strictly (prepare.py:624-627; here a ``ValueError``);
	* ``cadence``: the argument, else that of the sector (``sector``, or the sector in the first file's name) as
	  ``io.load_sector_settings`` gives it; a cadence ``prepare_frames`` has no smoothing width for is refused;
	* every frame's WCS goes through :func:`check_wcs_headers`; a frame that fails keeps the empty string (prepare.py:433-447);
	* the reference frame is the one nearest ``reference_time`` (BTJD; default: the middle of the time span) among the frames with
	  quality 0 and a good WCS (prepare.py:664-673); files without any WCS keywords skip the WCS part and choose among quality 0;
	* ``write``: path of a ``.tpstack`` that receives everything (``frameio.write_stack``): the groups ``images``, ``images_err``,
	  ``backgrounds``, ``pixel_flags``; time, cadenceno, quality, the offsets; the WCS strings with the reference frame's as
	  ``wcs_ref``; the movement kernel when computed; the attributes with ``SECTOR``, ``CADENCE``, ``TIME_OFFSET_CORRECTED = False``
	  and the vectors ``timecorr``, ``time_start``, ``time_stop``.  ``frameio.load_stack`` and ``motion.movement_from_header`` read it.

	Returns the dict of ``prepare_frames`` plus ``loaded``, ``wcs_headers``, ``ref_frame``, ``cadence`` and ``path``.
	"""
	from . import prepare, frameio
	loaded = files_or_loaded if isinstance(files_or_loaded, LoadedFFIs) else load_ffis(ctx, files_or_loaded, verify=verify)
	own = loaded is not files_or_loaded
	try:
		time = loaded.time
		if not np.all(time[:-1] < time[1:]):
			raise ValueError("Time vector is not sorted")
		if sector is None:
			sector = _sector_of(loaded.files[0])
		if cadence is None:
			if sector is None:
				raise ValueError("prepare_ffis: give cadence, or sector (the first file's name does not tell it)")
			cadence = sector_cadence(sector)
		if int(cadence) not in CADENCES:
			raise ValueError(f"prepare_ffis: no background smoothing width is defined for a cadence of {cadence} s (known: {', '.join(map(str, CADENCES))})")
		cadence = int(cadence)
		have_wcs = any(h.strip() for h in loaded.wcs_headers)
		if have_wcs:
			wcs_headers, bad_wcs = check_wcs_headers(ctx, loaded.wcs_headers)
		else:
			wcs_headers, bad_wcs = None, np.zeros(len(time), dtype=bool)
		if reference_time is None:
			reference_time = 0.5 * (time[0] + time[-1])
		ref = prepare._nearest_good_frame(time, np.where(bad_wcs, 1, loaded.quality), reference_time)
		if loaded.quality[ref] != 0 or bad_wcs[ref]:
			raise RuntimeError("The chosen refindx does not contain good values.")
		out = prepare.prepare_frames(ctx, loaded.raw, loaded.raw_err, loaded.quality, cadence=cadence, flux_cutoff=flux_cutoff, backapp=loaded.backapp,
			headers=loaded.headers, backgrounds_pixels_threshold=backgrounds_pixels_threshold, calc_movement_kernel=calc_movement_kernel, ref_frame=ref)
		out.update(loaded=loaded, wcs_headers=wcs_headers, ref_frame=ref, cadence=cadence, path=None)
		if write is not None:
			attrs = dict(loaded.attributes)
			attrs.update(SECTOR=sector, CADENCE=cadence, TIME_OFFSET_CORRECTED=False, timecorr=[float(v) for v in loaded.timecorr],
				time_start=[float(v) for v in loaded.time_start], time_stop=[float(v) for v in loaded.time_stop])
			groups = {name: out[name].to_host() for name in ('images', 'images_err', 'backgrounds', 'pixel_flags')}
			frameio.write_stack(write, groups, row_offset=loaded.row_offset, col_offset=loaded.col_offset, time=time, cadenceno=loaded.cadenceno,
				quality=loaded.quality, attrs=attrs, movement_kernel=out.get('movement_kernel'), movement_ref_frame=ref,
				wcs_headers=wcs_headers, wcs_ref=None if wcs_headers is None else wcs_headers[ref])
			out['path'] = write
		return out
	except BaseException:
		if own:
			loaded.free()
		raise
