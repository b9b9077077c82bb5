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
import struct
import time as _time
import zlib
from collections import namedtuple
import numpy as np
from . import fitsio
from . import inflate
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


class FFIHeader(namedtuple('FFIHeader', 'path header is_tess image uncert wcs_cards')):
	"""What :func:`read_ffi_header` returns (see there); ``hdus``, beside the tuple: the ``fitsio.HDU`` s it was made from."""
	hdus = ()


class InflateError(inflate.InflateError):
	"""A ``.gz`` file the device decoder (or, for a file that goes the host way, zlib) does not take to its end, or whose gzip CRC-32
	or ISIZE does not match: a ``ValueError`` that names the file and the status."""


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
	return _ffi_header(path, fitsio.scan_hdus(path, 3))


def read_ffi_header_from(path, read):
	"""
	:func:`read_ffi_header` from a source ``read(offset, n)`` of the file's (inflated) bytes instead of the file ``path`` (which only
	names it).  A source that holds the front of the file alone gives the headers in front of the first data unit: the
	:class:`FFIHeader` then has ``uncert = None``, and ``wcs_cards = None`` where HDU 1 lies behind that unit; what it has is what
	:func:`read_ffi_header` gives.  :func:`complete_ffi_header` adds the rest.
	"""
	return _ffi_header(str(path), fitsio.scan_hdus_from(read, 3, behind_data=False), front=True)


def complete_ffi_header(front, read):
	"""The whole :class:`FFIHeader` of a file whose front :func:`read_ffi_header_from` has read: ``read(offset, n)`` now gives the header
	blocks behind the image's data unit.  None where ``read`` does not reach that header's ``END`` card."""
	at = front.image.offset + front.image.nbytes
	behind = fitsio.scan_hdus_from(lambda offset, n: read(at + offset, n), 1)
	if not behind:
		return None
	hdus = list(front.hdus) + [u._replace(offset=u.offset + at) for u in behind]
	return _ffi_header(front.path, hdus)


def _ffi_header(path, scanned, front=False):
	"""What :func:`read_ffi_header` says, from the scanned HDUs; ``front``: they end with the first data unit."""
	hdus = []
	for n, u in enumerate(scanned):
		datasum = u.header.get('DATASUM')
		hdus.append((u.header, u.cards, DataUnit(n, u.offset, u.header.get('BITPIX'), u.shape, u.nbytes, None if datasum is None else int(str(datasum).strip()))))
	if front and len(hdus) == 1 and hdus[0][2].nbytes:
		# the image in the primary HDU: TESS or not is decided by HDU 1, which a TESS file has in front of its first data unit
		info = FFIHeader(path, dict(hdus[0][0]), False, hdus[0][2], None, None)
		info.hdus = list(scanned)
		return info
	if len(hdus) < 2:
		raise ValueError(f"{path}: an FFI has a primary HDU and at least one extension")
	hdr0, hdr1 = hdus[0][0], hdus[1][0]
	is_tess = hdr0.get('TELESCOP') == 'TESS' and hdr1.get('NAXIS1') == TESS_SHAPE[1] and hdr1.get('NAXIS2') == TESS_SHAPE[0]
	if is_tess:
		if len(hdus) < 3 and not front:
			raise ValueError(f"{path}: a TESS FFI has an image and an uncertainty extension")
		header = dict(hdr0)
		header.update(hdr1)
		if 'FFIINDEX' not in header and header['EXPOSURE'] * 86400 > 1000:
			header['FFIINDEX'] = extrapolate_ffiindex(header['TSTART'], header['TSTOP'], header.get('BARYCORR', 0))
		image, uncert = hdus[1][2], hdus[2][2] if len(hdus) > 2 else None
	else:
		header = dict(hdr0)
		image, uncert = hdus[0][2], hdus[1][2]
	info = FFIHeader(path, header, bool(is_tess), image, uncert, ''.join(hdus[1][1]))
	info.hdus = list(scanned)
	return info


def wcs_header_string(cards):
	"""The WCS keywords (and ``NAXIS1`` / ``NAXIS2``) of a string of 80-column cards, as a string of 80-column cards; '' without ``CTYPE1``."""
	keep = [cards[i:i + 80] for i in range(0, len(cards), 80) if cards[i + 8:i + 10] == '= ' and _WCS_KEY.match(cards[i:i + 8].strip())]
	if not any(c.startswith('CTYPE1 ') for c in keep):
		return ''
	return ''.join(c.ljust(80) for c in keep)


#--------------------------------------------------------------------------------------------------
def _check_units(h):
	"""The data units of one file: float images of one shape (a front without its uncertainty unit: the image alone)."""
	for unit in (h.image, h.uncert):
		if unit is not None and (unit.bitpix not in (-32, -64) or len(unit.shape) != 2):
			raise ValueError(f"{h.path}: HDU {unit.hdu} is not a float image (BITPIX {unit.bitpix}, shape {unit.shape}); integer images are not supported")
	if h.uncert is not None and h.image.shape != h.uncert.shape:
		raise ValueError(f"{h.path}: image {h.image.shape} and uncertainty {h.uncert.shape} differ in shape")


def load_ffis(ctx, files, verify=True, inflate='host', batch_files=None):
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

	``inflate='device'``: ``.gz`` files are not decompressed by the reader thread.  Their compressed bytes go through the same two
	staging buffers into a device area, ``batch_files`` files at a time (default: :func:`inflate_batch_files` of the free memory),
	one ``tp_inflate`` (csrc/inflate.hip, a wavefront per file) inflates the batch into slots sized from the gzip trailers' ISIZE, and
	``tp_fits_unpack`` / ``tp_fits_datasum`` read the inflated units in place.  The primary and the image header come from a host
	inflation of the file's first KBs, so the geometry is still checked before anything is allocated; the header behind the image
	unit (the uncertainty's) is downloaded from the inflated bytes, for the whole batch at once.  ``verify`` also holds the bytes to
	the gzip CRC-32 (formed on the device) and ISIZE.  A file with more than one gzip member, with other bytes behind the final block
	than the 8-byte trailer, or whose ISIZE is smaller than what its headers ask for goes the host way (logged at info level) with
	the same result; a stream the decoder does not take to its end, or a CRC-32 that does not match, raises :class:`InflateError`
	naming file and status.  Plain ``.fits`` files in the list go the way they always go; the result is the same bit for bit.
	``stats`` gains ``inflate_wait_s``, the seconds the host waited for the inflation, and ``inflate_files`` / ``host_files``.
	"""
	logger = logging.getLogger(__name__)
	files = [str(f) for f in files]
	if not files:
		raise ValueError("load_ffis: no files")
	if inflate not in ('host', 'device'):
		raise ValueError(f"load_ffis: inflate is 'host' or 'device', not {inflate!r}")
	fronts = {}                                                             # file number -> GzipFront of the files the device inflates
	host_files = 0                                                          # .gz files that go the host way although the device was asked for
	if inflate == 'device':
		infos = []
		for i, f in enumerate(files):
			front = gzip_front(f, i) if f.endswith('.gz') else None
			if front is not None and front.why_host is not None:
				logger.info("%s goes through the host's inflate: %s", f, front.why_host)
				front = None
				host_files += 1
			if front is None:
				infos.append(_host_header(f, i) if f.endswith('.gz') else read_ffi_header(f))
			else:
				fronts[i] = front
				infos.append(front.info)
	else:
		infos = [read_ffi_header(f) for f in files]
	first = infos[0]
	for h in infos:
		_check_units(h)
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
	out.row_offset, out.col_offset = 0, col0
	out.is_tess = is_tess
	out.files = files
	out.raw = out.raw_err = None

	# from the first byte of the image unit to the last of the uncertainty unit: what is read from a file
	# (a file the device inflates: its compressed bytes; should it go the host way after all, its two units and the blocks between)
	span = [(0, max(round_up(fronts[i].size, 4), 2 * h.image.nbytes + 16 * fitsio.BLOCK)) if i in fronts else _span(h) for i, h in enumerate(infos)]
	half = round_up(max(h.image.nbytes for h in infos), 256)            # every unit starts on a 256-byte boundary in device memory
	slot_bytes = half + round_up(max((h.uncert or h.image).nbytes for h in infos), 256)
	if batch_files is not None:
		batch_files = max(1, int(batch_files))
	elif fronts:
		batch_files = inflate_batch_files([f.size for f in fronts.values()], [f.pitch for f in fronts.values()], ctx.mem_info()[0] - 2 * T * R * C * 4)
	read_bytes = [0]
	tic = _time.perf_counter()
	try:
		out.raw = ctx.empty((T, R, C), 'float32')
		out.raw_err = ctx.empty((T, R, C), 'float32')
		with StagedUpload(ctx, max(n for _, n in span), slot_bytes, 2 * T if verify else 0) as st:
			up = st.up
			st.stats.update(inflate_wait_s=0.0, inflate_files=0, host_files=host_files)

			def unpack(i, h, d_image, d_uncert):
				for j, (unit, dst, d_unit) in enumerate(((h.image, out.raw, d_image), (h.uncert, out.raw_err, d_uncert))):
					if verify and unit.datasum is not None:
						st.datasum(d_unit, unit.nbytes, 2 * i + j)
					up._check(up.lib.tp_fits_unpack(up.handle, d_unit, unit.bitpix, unit.shape[1], unit.shape[0], row0, col0, R, C, dst.ptr + i * R * C * 4, C))

			def stage_file(i, h):
				"""File i through the reader: its two units as they lie in the (decompressed) file into the current slot."""
				begin, n = _span(h)
				if n > st.stage[0].nbytes or h.image.nbytes > half or h.uncert.nbytes > slot_bytes - half:
					raise ValueError(f"{h.path}: the units of the file ({n} bytes) are larger than its headers' front said")
				st.take()
				st.read(h.path, begin, n)
				for unit, d_unit in ((h.image, st.slot), (h.uncert, st.slot + half)):
					st.upload(d_unit, unit.nbytes, unit.offset - begin)
				st.record()
				unpack(i, h, st.slot, st.slot + half)
				read_bytes[0] += n

			batch = []
			for i, h in enumerate(infos):
				if i in fronts:
					batch.append(i)
				else:
					stage_file(i, h)
				if batch and (len(batch) == batch_files or i == T - 1):
					for k in _inflate_batch(ctx, st, batch, infos, fronts, verify, unpack, read_bytes):
						# (a file the device did not take: the host's inflate, with the same result or the host's own complaint)
						logger.info("%s goes through the host's inflate: %s", files[k], fronts[k].why_host)
						infos[k] = _host_header(files[k], k)
						_check_units(infos[k])
						if infos[k].is_tess != first.is_tess or infos[k].image.shape != first.image.shape:
							raise ValueError(f"{files[k]}: shape {infos[k].image.shape} (TESS: {infos[k].is_tess}) differs from that of {first.path}")
						try:
							stage_file(k, infos[k])
						except (EOFError, OSError, zlib.error) as e:
							raise InflateError(k, 'HOST', f"{files[k]}: the host's inflate fails: {e}") from e
						st.stats['host_files'] += 1
					batch = []
			sums = st.finish()
		if verify:
			for i, h in enumerate(infos):
				for j, unit in enumerate((h.image, h.uncert)):
					check_datasum(h.path, unit.hdu, sums[2 * i + j], unit.datasum)
	except BaseException:
		out.free()                                                      # (the transfer context has been synced: nothing can write into the stacks any more)
		raise
	out.wcs_headers = [wcs_header_string(h.wcs_cards) for h in infos]
	out.stats = dict(st.stats, bytes=int(read_bytes[0]), total_s=_time.perf_counter() - tic)
	return out


def _span(h):
	"""From the first byte of the image unit to the last of the uncertainty unit: what the reader takes from a file."""
	return h.image.offset, h.uncert.offset + h.uncert.nbytes - h.image.offset


#--------------------------------------------------------------------------------------------------
#: inflated bytes of a file's front the host looks at for the primary and the image header, and the compressed bytes it reads for them
FRONT_INFLATED = 32 * fitsio.BLOCK
FRONT_COMPRESSED = 256 << 10
#: 2880-byte blocks downloaded per file for the header behind the image unit (more where END is not among them)
HEADER_BLOCKS = 4
#: the share of the free device memory a batch's compressed and inflated bytes may take, and the most files of a batch
INFLATE_BATCH_SHARE = 0.5
INFLATE_BATCH_MAX = 1024


def inflate_batch_files(compressed_sizes, inflated_sizes, free_bytes, share=INFLATE_BATCH_SHARE, most=INFLATE_BATCH_MAX):
	"""
	Files per ``tp_inflate`` launch of ``load_ffis(inflate='device')`` from the files' compressed and inflated sizes: as many of the
	largest file's compressed and inflated bytes (each rounded up to 256) as fit ``share`` of ``free_bytes``; at least 1, at most
	``most`` and the number of files.  One wavefront inflates a file, so a batch pays off with hundreds of files.
	"""
	per_file = max(round_up(int(c), 256) for c in compressed_sizes) + max(round_up(int(n), 256) for n in inflated_sizes)
	return int(max(1, min(int(most), len(compressed_sizes), int(share * max(free_bytes, 0)) // max(per_file, 1))))


class GzipFront(object):
	"""
	What the host learns from the front and the last 8 bytes of a ``.gz`` file (:func:`gzip_front`): ``size`` of the file, ``begin`` of
	the deflate stream, the trailer's ``crc`` and ``isize``, ``pitch`` (the slot of its inflated bytes: ISIZE rounded up to 256),
	``info`` (the :class:`FFIHeader` of :func:`read_ffi_header_from`) and ``why_host``: None, or why the device path does not take it.
	"""

	def __init__(self, path, index):
		self.path, self.index, self.why_host, self.info = path, index, None, None
		self.size = os.path.getsize(path)
		with open(path, 'rb') as fh:
			head = fh.read(min(self.size, FRONT_COMPRESSED))
			fh.seek(max(self.size - 8, 0))
			tail = fh.read(8)
		self.begin = inflate.header_length(head, index)
		if self.size < self.begin + 8:
			raise inflate.InflateError(index, 'FRAMING')
		self.crc, self.isize = struct.unpack('<II', tail)
		self.pitch = round_up(self.isize, 256)
		d = zlib.decompressobj(-15)
		front = d.decompress(head[self.begin:], FRONT_INFLATED)
		if d.eof and (len(d.unused_data) > 8 or len(head) < self.size):
			self.why_host = 'its first member ends in the front of the file, and is not the last one'
			return
		self.info = read_ffi_header_from(path, lambda offset, n: front[offset:offset + n])
		need = self.info.image.offset + self.info.image.nbytes + fitsio.BLOCK
		if self.isize < need:
			self.why_host = f'its last member holds {self.isize} bytes where the headers ask for {need} and more'
		elif self.isize > inflate.MAX_RATIO * (self.size - self.begin - 8) + 16:
			raise inflate.InflateError(index, 'ISIZE')


def gzip_front(path, index=0):
	"""The :class:`GzipFront` of the ``.gz`` file ``path``; :class:`InflateError` naming the file where its front is no gzip member that
	inflates, ``ValueError`` where the inflated front is no FFI."""
	try:
		return GzipFront(path, index)
	except (inflate.InflateError, zlib.error) as e:
		raise InflateError(index, getattr(e, 'status', 'FRAMING'), f"{path}: {getattr(e, 'status', e)}: the front of the file does not inflate") from e


def _host_header(path, index):
	try:
		return read_ffi_header(path)
	except (EOFError, OSError, zlib.error) as e:
		raise InflateError(index, 'HOST', f"{path}: the host's inflate fails: {e}") from e


def _inflate_batch(ctx, st, batch, infos, fronts, verify, unpack, read_bytes):
	"""
	The files ``batch`` (file numbers with a :class:`GzipFront`) of ``load_ffis(inflate='device')``: compressed bytes up through the
	staging buffers, one ``tp_inflate``, the headers behind the image units down in one go, ``unpack(i, header, d_image, d_uncert)``
	on the inflated units in place.  ``infos[i]`` becomes the file's whole header.  Returns the file numbers that have to go the host
	way; raises :class:`InflateError` for a broken one.  The batch's device areas are gone when it returns or raises.
	"""
	up, lib = st.up, st.up.lib
	n = len(batch)
	f = [fronts[i] for i in batch]
	c_off = np.zeros(n + 1, dtype='uint64')
	c_off[1:] = np.cumsum([round_up(x.size, 256) for x in f], dtype='uint64')
	o_off = np.zeros(n + 1, dtype='uint64')
	o_off[1:] = np.cumsum([x.pitch for x in f], dtype='uint64')
	# tp_inflate takes adjacent streams: file k is stream 2k, the bytes between its final block and the next file's stream (trailer,
	# padding, gzip header) are stream 2k + 1 with a slot of no bytes, which is refused at its first byte and writes nothing
	in_offsets = np.zeros(2 * n + 1, dtype='uint64')
	out_offsets = np.zeros(2 * n + 1, dtype='uint64')
	for k, x in enumerate(f):
		in_offsets[2 * k] = int(c_off[k]) + x.begin
		in_offsets[2 * k + 1] = int(c_off[k]) + x.size - 8
		out_offsets[2 * k] = o_off[k]
		out_offsets[2 * k + 1] = o_off[k + 1]
	in_offsets[2 * n] = int(c_off[n - 1]) + f[-1].size
	out_offsets[2 * n] = o_off[n]
	m = 2 * n
	d_comp = d_inf = d_meta = meta = heads = None
	to_host = []
	try:
		d_comp = ctx.empty(max(int(c_off[n]), 256), 'uint8')
		d_inf = ctx.empty(max(int(o_off[n]), 256), 'uint8')
		d_meta = ctx.empty(24 * m, 'uint8')                                # produced and consumed (uint64 each), statuses (int32), CRCs (uint32)
		meta = ctx.pinned((24 * m,), 'uint8')
		for k, x in enumerate(f):
			st.take()
			st.fill(lambda buf, x=x: _read_raw(x.path, buf, x.size))
			st.upload(d_comp.ptr + int(c_off[k]), round_up(x.size, 4))
			st.record()
			read_bytes[0] += x.size
		up._check(lib.tp_inflate(up.handle, d_comp.ptr, in_offsets.ctypes.data, m, d_inf.ptr, out_offsets.ctypes.data, d_meta.ptr + 16 * m, d_meta.ptr, d_meta.ptr + 8 * m,
			d_meta.ptr + 20 * m))
		up.download_async(meta, d_meta, nbytes=24 * m)
		t0 = _time.perf_counter()
		up.sync()
		st.stats['inflate_wait_s'] += _time.perf_counter() - t0
		produced = meta.array[:8 * m].view('uint64')[0::2]
		consumed = meta.array[8 * m:16 * m].view('uint64')[0::2]
		statuses = meta.array[16 * m:20 * m].view('int32')[0::2]
		crcs = meta.array[20 * m:24 * m].view('uint32')[0::2]
		taken = []
		for k, x in enumerate(f):
			name = inflate.status_name(statuses[k])
			if statuses[k] == inflate.OK and int(consumed[k]) < x.size - 8 - x.begin:
				x.why_host = 'bytes lie between its final block and its last 8 bytes (more than one member, or padding)'
			elif statuses[k] == inflate.OK and int(produced[k]) != x.isize:
				raise InflateError(batch[k], 'ISIZE', f"{x.path}: ISIZE: {int(produced[k])} bytes where the trailer says {x.isize}")
			elif name == 'OUTPUT_FULL':
				x.why_host = 'it holds more bytes than its last 8 bytes say (more than one member?)'
			elif statuses[k] != inflate.OK:
				raise InflateError(batch[k], name, f"{x.path}: {name}: the deflate stream is broken {int(produced[k])} bytes into the file")
			elif verify and int(crcs[k]) != x.crc:
				raise InflateError(batch[k], 'CRC', f"{x.path}: CRC: the inflated bytes have CRC-32 {int(crcs[k]):08x}, the trailer says {x.crc:08x}")
			if x.why_host is None:
				taken.append(k)
			else:
				to_host.append(batch[k])
		# the header behind the image unit, for every file of the batch in one go; more blocks where END is not among the first ones
		blocks = HEADER_BLOCKS
		while taken:
			at = [int(o_off[k]) + f[k].info.image.offset + f[k].info.image.nbytes for k in taken]
			room = [min(blocks * fitsio.BLOCK, f[k].isize - (f[k].info.image.offset + f[k].info.image.nbytes)) for k in taken]
			heads = ctx.pinned((len(taken) * blocks * fitsio.BLOCK,), 'uint8')
			for j, (a, r) in enumerate(zip(at, room)):
				up._check(lib.tp_memcpy_d2h_async(up.handle, heads.ptr + j * blocks * fitsio.BLOCK, d_inf.ptr + a, r))
			up.sync()
			short = []
			for j, k in enumerate(taken):
				mine = bytes(heads.array[j * blocks * fitsio.BLOCK:j * blocks * fitsio.BLOCK + room[j]])
				whole = complete_ffi_header(f[k].info, lambda offset, n_, mine=mine, base=f[k].info.image.offset + f[k].info.image.nbytes: mine[offset - base:offset - base + n_])
				if whole is None:
					if room[j] < blocks * fitsio.BLOCK:
						raise ValueError(f"{f[k].path}: no header behind the image's data unit")
					short.append(k)
					continue
				_check_units(whole)
				if whole.is_tess != f[k].info.is_tess or whole.image != f[k].info.image:
					raise ValueError(f"{f[k].path}: the headers behind the image unit make it another kind of file than those in front")
				infos[batch[k]] = whole
				if whole.uncert.offset + whole.uncert.nbytes > f[k].isize:
					f[k].why_host = f'its last member holds {f[k].isize} bytes where the headers ask for {whole.uncert.offset + whole.uncert.nbytes}'
					to_host.append(batch[k])
					continue
				unpack(batch[k], whole, d_inf.ptr + int(o_off[k]) + whole.image.offset, d_inf.ptr + int(o_off[k]) + whole.uncert.offset)
				st.stats['inflate_files'] += 1
			heads.free()
			heads = None
			taken, blocks = short, 4 * blocks
		return sorted(to_host)
	finally:
		try:
			up.sync()                                                       # the kernels that read the batch's areas are over
		except Exception: # noqa: B902
			pass
		for d in (d_comp, d_inf, d_meta, meta, heads):
			if d is not None:
				d.free()


def _read_raw(path, buf, nbytes):
	"""The file's own bytes into the uint8 array ``buf``."""
	view = memoryview(buf)[:nbytes]
	with open(path, 'rb') as fh:
		got = 0
		while got < nbytes:
			k = fh.readinto(view[got:])
			if not k:
				raise ValueError(f"{path}: the file has shrunk to {got} of {nbytes} bytes")
			got += k


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
	flux_cutoff=8e4, backgrounds_pixels_threshold=0.5, inflate='host', batch_files=None):
	"""
	The prepare stage from FFI files to prepared stacks: :func:`load_ffis` (unless a :class:`LoadedFFIs` is given; ``inflate`` and ``batch_files`` are its),
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
	loaded = files_or_loaded if isinstance(files_or_loaded, LoadedFFIs) else load_ffis(ctx, files_or_loaded, verify=verify, inflate=inflate,
		batch_files=batch_files)
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
