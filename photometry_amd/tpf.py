# -*- coding: utf-8 -*-
"""
Target pixel files (``*_tp.fits``, ``*_fast-tp.fits``) into device-resident stamp cubes: the input side of a ``datasource='tpf'`` run.

The reference opens a TPF with astropy (BasePhotometry.py:320-384): the ``TIME`` / ``TIMECORR`` / ``CADENCENO`` / ``QUALITY`` /
``POS_CORR1,2`` columns of the ``PIXELS`` table with the rows of non-finite ``TIME`` dropped, the ``APERTURE`` image with its WCS and
the stamp's place on the CCD, a few cards, and -- row by row, ``cube[:, :, k] = data[field][k]`` (``_load_cube``, :720-751) -- the
``FLUX``, ``FLUX_ERR`` and ``FLUX_BKG`` columns as ``(rows, cols, times)`` cubes.  Here the header blocks are parsed on the host
(``fitsio.read_header_blocks``), the scalar columns are read on the host through strided big-endian views (a few hundred kB), the
table's data unit travels over the link exactly as it lies in the file, and the byte swap and the transposition of the three image
columns into ``[H][W][t_pitch]`` cubes happen in HBM in one launch (``tp_tpf_unpack``, csrc/tpfin.hip).  The table's ``DATASUM`` is
checked on the device with ``tp_fits_datasum``.

:func:`find_tpf_files` is the reference's file-name rule, :func:`read_tpf_header` what the headers alone tell, :func:`load_tpfs`
the streaming loader, :func:`time_offset` the timestamp fix of the early data releases (fixes/time_offset.py), which this loader
applies as the reference does at BasePhotometry.py:384, and :class:`TpfStampSource` hands a loaded file to the plugin classes.
:func:`load_tpf_groups` is the loader of a batched run (``tessphot_tpfs``): the same stream into one set of cubes per group of files
that share ``(H, W, T)`` -- ``TIME`` is barycentric per target, so a group shares its shape and nothing else, and carries a time and a
quality vector per file; :func:`plan_groups` is where every file ends up, :func:`project_for_files` and :func:`main_targets` make
catalogue and main target of every file what :class:`TpfStampSource` would.

Not covered: image columns other than
``E``, ``RAW_CNTS`` and ``FLUX_BKG_ERR``, the pixel-quality and cosmic-ray extensions, the HDF5-side inputs of a ``tpf`` run in the
reference (the catalogue comes in as a dict), tile-compressed files.
"""

import ctypes
import logging
import os
import re
from collections import namedtuple, defaultdict
import numpy as np
from . import fitsio
from . import ffi
from .device import DeviceCube, round_up
from .source import MemoryStampSource
from .staging import StagedUpload, check_datasum

#: the columns of the PIXELS table the loader reads, and those among them that are images
COLUMNS = ('TIME', 'TIMECORR', 'CADENCENO', 'FLUX', 'FLUX_ERR', 'FLUX_BKG', 'QUALITY', 'POS_CORR1', 'POS_CORR2')
IMAGE_COLUMNS = (('images', 'FLUX'), ('images_err', 'FLUX_ERR'), ('backgrounds', 'FLUX_BKG'))
#: bytes per element of a TFORM letter
_TFORM_BYTES = {'L': 1, 'B': 1, 'A': 1, 'I': 2, 'J': 4, 'K': 8, 'E': 4, 'D': 8, 'C': 8, 'M': 16}
#: numpy codes of the scalar columns
_SCALAR = {'TIME': ('D', '>f8'), 'TIMECORR': ('E', '>f4'), 'CADENCENO': ('J', '>i4'), 'QUALITY': ('J', '>i4'), 'POS_CORR1': ('E', '>f4'), 'POS_CORR2': ('E', '>f4')}

#: a column of the table: name, TFORM, bytes into a row, TDIM (fastest axis first) or None
TableColumn = namedtuple('TableColumn', 'name tform offset tdim')
#: the PIXELS table: HDU number, byte offset of the data unit, its bytes with the padding, NAXIS1, NAXIS2, DATASUM (or None), columns by name, header
TableLayout = namedtuple('TableLayout', 'hdu offset nbytes row_bytes n_rows datasum columns header')
#: the APERTURE image: HDU number, header, raw cards, byte offset and padded bytes of its data unit, BITPIX, (NAXIS2, NAXIS1)
ApertureUnit = namedtuple('ApertureUnit', 'hdu header cards offset nbytes bitpix shape')
TPFHeader = namedtuple('TPFHeader', 'path header table aperture')


class LoadedTPF(object):
	"""What :func:`load_tpfs` returns per file (see there); ``free()`` releases the three cubes."""

	def free(self):
		cubes = self.__dict__.get('cubes') or {}
		for name in list(cubes):
			if cubes[name] is not None:
				cubes[name].free()
			cubes[name] = None


#--------------------------------------------------------------------------------------------------
def find_tpf_files(rootdir, starid=None, sector=None, camera=None, ccd=None, cadence=None, findmax=None):
	"""
	Full paths of the target pixel files below ``rootdir`` (searched recursively, links followed), optionally of one star, sector,
	camera, CCD or cadence: the rule of io.py:170-280.  Two file-name patterns: SPOC's ``tess<time>-s<sector>-<starid>-<4
	digits>-<x|s|a|b>_tp.fits`` (``_fast-tp.fits`` for the 20 s cadence; ``cadence=None`` takes both) and, for ``cadence`` None or
	120, the TESS-alert ``hlsp_tess-data-alerts_tess_phot_<starid>-s<2-digit sector>_tess_v<n>_tp.fits``; either optionally
	``.gz``.  Each star's files are sorted by base name, and so is the whole list without ``starid``.  ``camera`` / ``ccd`` read the
	primary header of every candidate (header blocks only).  ``findmax`` cuts the list.  Not cached: a second call sees what has
	changed on disk.
	"""
	if cadence is not None and cadence not in (120, 20):
		raise ValueError("Invalid cadence. Must be either 20 or 120.")
	sector_str = r'\d{4}' if sector is None else f'{int(sector):04d}'
	suffix = {None: '(fast-)?tp', 120: 'tp', 20: 'fast-tp'}[cadence]
	regexps = [re.compile(r'^tess\d+-s(?P<sector>' + sector_str + r')-(?P<starid>\d+)-\d{4}-[xsab]_' + suffix + r'\.fits(\.gz)?$')]
	if cadence is None or cadence == 120:
		sector_str = r'\d{2}' if sector is None else f'{int(sector):02d}'
		regexps.append(re.compile(r'^hlsp_tess-data-alerts_tess_phot_(?P<starid>\d+)-s(?P<sector>' + sector_str + r')_tess_v\d+_tp\.fits(\.gz)?$'))
	filedict = defaultdict(list)
	for root, _, filenames in os.walk(rootdir, followlinks=True):
		for filename in filenames:
			for regex in regexps:
				m = regex.match(filename)
				if m:
					filedict[int(m.group('starid'))].append(os.path.join(root, filename))
					break
	for key in filedict:
		filedict[key].sort(key=os.path.basename)
	if starid is not None:
		files = list(filedict.get(int(starid), []))
	else:
		files = [f for lst in filedict.values() for f in lst]
		files.sort(key=os.path.basename)
	if camera is not None or ccd is not None:
		matches = []
		for fpath in files:
			hdr = _primary_header(fpath)
			if camera is not None and hdr.get('CAMERA') != camera:
				continue
			if ccd is not None and hdr.get('CCD') != ccd:
				continue
			matches.append(fpath)
			if findmax is not None and len(matches) >= findmax:
				break
		files = matches
	if findmax is not None and len(files) > findmax:
		files = files[:findmax]
	return files


def _primary_header(path):
	return fitsio.scan_hdus(path, 1)[0].header


#--------------------------------------------------------------------------------------------------
def _table_columns(path, header):
	"""The columns of a binary-table header by name, with their byte offsets; their sizes have to add up to NAXIS1."""
	columns, offset = {}, 0
	for i in range(1, int(header.get('TFIELDS', 0)) + 1):
		tform = str(header.get(f'TFORM{i}', '')).strip()
		m = re.fullmatch(r'(\d*)([A-Z])(\(.*\))?', tform)
		if m is None or m.group(2) not in _TFORM_BYTES:
			raise ValueError(f"{path}: column {i} of the PIXELS table has the TFORM {tform!r}, which is not understood")
		name = str(header.get(f'TTYPE{i}', f'COL{i}')).strip()
		tdim = header.get(f'TDIM{i}')
		columns[name] = TableColumn(name, tform, offset, None if tdim is None else tuple(int(v) for v in str(tdim).strip().strip('()').split(',')))
		offset += (int(m.group(1)) if m.group(1) else 1) * _TFORM_BYTES[m.group(2)]
	if offset != header.get('NAXIS1'):
		raise ValueError(f"{path}: the columns of the PIXELS table add up to {offset} bytes, NAXIS1 says {header.get('NAXIS1')}")
	return columns


def read_tpf_header(path):
	"""
	What the reference takes from the headers of a TPF, reading header blocks only (the data units are skipped with ``seek``, so a
	file cut short behind its last header still answers).  Returns a :class:`TPFHeader`:

	``header``: the primary header (BasePhotometry.py:330).
	``table``: the :class:`TableLayout` of the ``PIXELS`` table (HDU 1): where its data unit lies, ``NAXIS1`` / ``NAXIS2``, its
	``DATASUM``, its header, and every column as a :class:`TableColumn`.
	``aperture``: the :class:`ApertureUnit` of the ``APERTURE`` image (HDU 2): header, raw cards, where its data unit lies.

	``ValueError`` naming the file: one of :data:`COLUMNS` is missing or a scalar one has another type than the TESS files give it,
	an image column is not ``E``, the three image columns differ in ``TDIM``, ``TDIM`` disagrees with ``NAXIS1`` / ``NAXIS2`` of
	the APERTURE image.
	"""
	path = str(path)
	hdus = fitsio.scan_hdus(path, 3)
	if len(hdus) < 3:
		raise ValueError(f"{path}: a target pixel file has a primary HDU, the PIXELS table and the APERTURE image")
	thdr, _, toff, tbytes, _ = hdus[1]
	ahdr, acards, aoff, abytes, ashape = hdus[2]
	if thdr.get('XTENSION') != 'BINTABLE' or thdr.get('NAXIS') != 2:
		raise ValueError(f"{path}: HDU 1 is not a binary table")
	if ahdr.get('XTENSION') != 'IMAGE' or len(ashape) != 2:
		raise ValueError(f"{path}: HDU 2 is not a two-dimensional image")
	columns = _table_columns(path, thdr)
	for name in COLUMNS:
		if name not in columns:
			raise ValueError(f"{path}: the PIXELS table has no column {name}")
	for name, (letter, _) in _SCALAR.items():
		if columns[name].tform != letter:
			raise ValueError(f"{path}: column {name} has the TFORM {columns[name].tform!r}, not {letter!r}")
	first = columns[IMAGE_COLUMNS[0][1]]
	for _, name in IMAGE_COLUMNS:
		col = columns[name]
		if not re.fullmatch(r'\d*E', col.tform):
			raise ValueError(f"{path}: image column {name} has the TFORM {col.tform!r}; only E (float32) image columns are supported")
		if col.tdim is None or len(col.tdim) != 2:
			raise ValueError(f"{path}: image column {name} has no two-dimensional TDIM")
		if col.tdim != first.tdim:
			raise ValueError(f"{path}: image column {name} has the TDIM {col.tdim}, {first.name} has {first.tdim}")
		repeat = int(col.tform[:-1] or 1)
		if repeat != col.tdim[0] * col.tdim[1]:
			raise ValueError(f"{path}: image column {name}: TFORM {col.tform!r} does not hold TDIM {col.tdim}")
	if first.tdim != (ahdr.get('NAXIS1'), ahdr.get('NAXIS2')):
		raise ValueError(f"{path}: the image columns have the TDIM {first.tdim}, the APERTURE image is {ahdr.get('NAXIS1')} x {ahdr.get('NAXIS2')}")
	datasum = thdr.get('DATASUM')
	table = TableLayout(1, toff, tbytes, int(thdr['NAXIS1']), int(thdr['NAXIS2']), None if datasum is None else int(str(datasum).strip()), columns, thdr)
	aperture = ApertureUnit(2, ahdr, ''.join(acards), aoff, abytes, ahdr.get('BITPIX'), ashape)
	return TPFHeader(path, hdus[0][0], table, aperture)


#--------------------------------------------------------------------------------------------------
def time_offset(time, header, datatype='tpf', timepos='mid', return_flag=False):
	"""
	The timestamp correction of the early data releases, fixes/time_offset.py:95-180: ``DATA_REL <= 26`` always, 27 and 29 for the
	``PROCVER`` values of their first releases (without ``PROCVER``: ``ValueError``), nothing beyond 29 or when the header says
	``TIME_OFFSET_CORRECTED``.  Mid-times move by ``-2.000 + 0.021`` s, start times by ``-2.000 + 0.031`` s, end times by ``-2.000 +
	0.011`` s; for ``datatype='ffi'`` of ``DATA_REL <= 26`` (and the first release 27) the staggered readout of camera and CCD is
	added.  ``[fixes] time_offset = false`` in the settings (``plugins.load_settings``) turns the fix off with a warning.  Returns the times, with ``return_flag`` also whether they were corrected.
	"""
	logger = logging.getLogger(__name__)
	datarel = int(header['DATA_REL'])
	procver = header.get('PROCVER', None)
	already_corrected = bool(header.get('TIME_OFFSET_CORRECTED', False))
	if timepos not in ('start', 'mid', 'end'):
		raise ValueError("Invalid TIMEPOS")
	first_release_27 = False
	if already_corrected or datarel > 29:
		apply = False
	elif datarel <= 26:
		apply = True
	elif datarel in (27, 29) and procver is None:
		raise ValueError("The timestamps of these data may need to be corrected, but the PROCVER header is not present.")
	elif datarel == 27 and procver in ('spoc-4.0.14-20200108', 'spoc-4.0.15-20200114', 'spoc-4.0.17-20200130'):
		first_release_27 = True
		apply = True
	elif datarel == 29 and procver in ('spoc-4.0.17-20200130', 'spoc-4.0.20-20200220', 'spoc-4.0.21-20200227'):
		apply = True
	else:
		apply = False
	if apply:
		from .plugins import load_settings
		if not load_settings().getboolean('fixes', 'time_offset', fallback=True):
			logger.warning("SettingsWarning: Time offset fix has been turned off in settings.")
			apply = False
	if apply:
		staggered = 0
		if datatype == 'ffi' and (datarel <= 26 or first_release_27):
			staggered = {1: 0.000, 2: 1.500, 3: 0.500, 4: 1.000}[int(header['CAMERA'])]
			staggered += {1: 0.000, 2: 0.020, 3: 0.040, 4: 0.060}[int(header['CCD'])]
		time = time + (staggered - 2.000 + {'mid': 0.021, 'start': 0.031, 'end': 0.011}[timepos]) / 86400
	return (time, apply) if return_flag else time


#--------------------------------------------------------------------------------------------------
def _column_view(buf, table, name, base):
	"""Column ``name`` of the table whose data unit begins ``base`` bytes into the uint8 array ``buf``: a strided big-endian view."""
	return np.ndarray((table.n_rows,), dtype=_SCALAR[name][1], buffer=buf, offset=base + table.columns[name].offset, strides=(table.row_bytes,))


def load_tpfs(ctx, files, verify=True):
	"""
	Load the target pixel files ``files`` (in the order given); returns one :class:`LoadedTPF` per file with

	``cubes``: ``{'images', 'images_err', 'backgrounds'}``, float32 :class:`~photometry_amd.device.DeviceCube` s of one target
	``(1, T, H, W)`` from ``FLUX`` / ``FLUX_ERR`` / ``FLUX_BKG`` (BasePhotometry.py:720-751), made on ``ctx``;
	``time`` (float64, with :func:`time_offset` applied as at BasePhotometry.py:384; ``time_offset_corrected`` says whether it changed
	anything), ``timecorr`` (float32 as in the file, :344), ``cadenceno``, ``quality`` (int32), ``pos_corr`` ``(T, 2)`` float64 from
	``POS_CORR1`` / ``POS_CORR2`` (:471) -- all without the rows whose ``TIME`` is not finite (:339-340); ``rows_dropped`` counts them;
	``aperture``: the APERTURE image, int32 ``(H, W)``, as in the file; ``max_stamp``: ``(CRVAL2P - 1, CRVAL2P - 1 + NAXIS2, CRVAL1P - 1,
	CRVAL1P - 1 + NAXIS1)`` of its header (:354-359); ``wcs_cards``: the WCS keywords of that header (``ffi.wcs_header_string``);
	``header``: the primary header; ``sector``, ``camera``, ``ccd``, ``data_rel`` from it; ``cadence``: ``round(TIMEDEL * 86400)`` of
	the table header (:335); ``readnoise``, ``gain``, ``num_frm``, ``n_readout``: ``READNOIA`` / ``GAINA`` / ``NUM_FRM`` / ``NREADOUT`` of
	the table header with the reference's defaults 10 / 100 / 60 / 48 (:370-373); ``path``; ``stats``: seconds the host spent reading
	and waiting for this file, and its bytes.

	Every header is read and checked (:func:`read_tpf_header`) before anything is allocated.  The files then stream through two
	page-locked staging buffers on a second context (``staging.StagedUpload``): while file ``i`` transfers and unpacks, file
	``i + 1`` is read (``readinto``; a ``.gz`` is decompressed) straight into the other buffer.  The scalar columns are read out of the
	staging buffer on the host, so the size of the cubes is known without a device round trip.  ``verify``: the word sum of every
	table that has a ``DATASUM`` card is formed on the device and compared once all files are in; a mismatch raises
	``ffi.ChecksumError`` naming file and HDU.  After any exception the staging buffers, events and all cubes are gone.
	"""
	files = [str(f) for f in files]
	if not files:
		raise ValueError("load_tpfs: no files")
	infos = [read_tpf_header(f) for f in files]
	_check_aperture_units(infos)
	loaded = []

	def fresh_cubes(i, out):
		"""A one-target cube per image column of file ``i``, its pitch from ``T``."""
		H, W = out.aperture.shape
		for name in out.cubes:
			out.cubes[name] = DeviceCube(ctx, 1, len(out.time), H, W)
		return [cube.ptr for cube in out.cubes.values()], out.cubes['images'].t_pitch
	try:
		with _staging(ctx, infos, verify) as st:
			_stream_files(st, infos, verify, loaded, fresh_cubes)
			sums = st.finish()
		if verify:
			for h, got in zip(infos, sums):
				check_datasum(h.path, h.table.hdu, got, h.table.datasum)
	except BaseException:
		for out in loaded:
			out.free()                                                   # (the transfer context has been synced: nothing can write into a cube any more)
		raise
	return loaded


def _span(h):
	"""``(first byte, bytes)`` of what is read from a file: from the first byte of the table to the last of the APERTURE image."""
	return h.table.offset, h.aperture.offset + h.aperture.nbytes - h.table.offset


def _staging(ctx, infos, verify):
	"""The :class:`~photometry_amd.staging.StagedUpload` of a run over ``infos``: a slot holds a table, sum ``i`` is that of file ``i``."""
	return StagedUpload(ctx, max(_span(h)[1] for h in infos), round_up(max(h.table.nbytes for h in infos), 256), len(infos) if verify else 0)


def _stream_files(st, infos, verify, loaded, place):
	"""
	The per-file body of :func:`load_tpfs` and :func:`load_tpf_groups`: every file of ``infos`` through the staging buffers of ``st``
	(``staging``: while file ``i`` transfers and unpacks, file ``i + 1`` is read), its :class:`LoadedTPF` without cubes appended to
	``loaded``, its table summed and its three image columns unpacked to where ``place(i, out)`` says: the device addresses of the
	three columns of file ``i`` and their ``t_pitch``.
	"""
	up = st.up
	for i, h in enumerate(infos):
		tb = h.table
		start, nbytes = _span(h)
		st.stats = {'read_s': 0.0, 'wait_s': 0.0, 'bytes': int(nbytes)}
		st.take()
		st.read(h.path, start, nbytes)
		st.upload(st.slot, tb.nbytes)
		st.record()
		out = _host_side(h, st.buf.array)                                # (the host reads the staging buffer while the DMA does)
		out.stats = st.stats
		out.cubes = {name: None for name, _ in IMAGE_COLUMNS}
		loaded.append(out)
		H, W = out.aperture.shape
		T = len(out.time)
		if T == 0:
			raise ValueError(f"{h.path}: no row of the PIXELS table has a finite TIME")
		dst, t_pitch = place(i, out)
		if verify and tb.datasum is not None:
			st.datasum(st.slot, tb.nbytes, i)
		rows = None if out.rows_dropped == 0 else np.ascontiguousarray(out._kept_rows, dtype='int32')
		offsets = (ctypes.c_int64 * 3)(*[tb.columns[col].offset for _, col in IMAGE_COLUMNS])
		outs = (ctypes.c_void_p * 3)(*dst)
		up._check(up.lib.tp_tpf_unpack(up.handle, st.slot, tb.row_bytes, tb.n_rows, None if rows is None else rows.ctypes.data, T, 3,
			ctypes.addressof(offsets), H * W, ctypes.addressof(outs), t_pitch))
		del out._kept_rows


#--------------------------------------------------------------------------------------------------
class TpfGroup(object):
	"""
	The files of one :func:`load_tpf_groups` call that share ``(H, W, T)``, in one cube per image column:

	``shape``: ``(H, W, T)``; ``cubes``: ``{'images', 'images_err', 'backgrounds'}``, :class:`~photometry_amd.device.DeviceCube` s of
	``n`` targets; ``loaded``: one :class:`LoadedTPF` per slot, its ``cubes`` non-owning one-target views of its slot (``free()`` on
	them releases nothing); ``time`` ``(n, T)`` float64, ``quality`` ``(n, T)`` int32, ``aperture`` ``(n, H, W)`` int32 without the
	flags of SPOC's mask (2) and centroid pixels (8), as ``BasePhotometry.aperture`` takes them for a ``tpf`` run.  ``free()``
	releases the cubes of the group.
	"""

	def __init__(self, shape, cubes, owned, loaded):
		self.shape = tuple(int(v) for v in shape)
		self.cubes, self._owned, self.loaded = cubes, owned, loaded
		self.time = np.stack([ld.time for ld in loaded]).astype('float64')
		self.quality = np.stack([ld.quality for ld in loaded]).astype('int32')
		self.aperture = np.stack([ld.aperture for ld in loaded]).astype('int32') & ~np.int32(2 | 8)

	def __len__(self):
		return len(self.loaded)

	def free(self):
		for ld in self.loaded:
			ld.free()
		for cube in self._owned:
			cube.free()
		self._owned = []
		self.cubes = {name: None for name in self.cubes}


def bucket_files(shapes):
	"""``shapes``: ``(H, W, n_rows)`` of every file, from the headers.  Returns ``(keys, members)``: the distinct shapes in the order of
	their first file and, per shape, its files in the order given -- file ``members[b][j]`` is unpacked into slot ``j`` of bucket ``b``."""
	keys, members = [], []
	for i, s in enumerate(shapes):
		s = tuple(int(v) for v in s)
		if s not in keys:
			keys.append(s)
			members.append([])
		members[keys.index(s)].append(i)
	return keys, members


def plan_groups(shapes, kept):
	"""
	Where the files of :func:`load_tpf_groups` end up: a pure function of the header shapes ``(H, W, n_rows)`` and of ``kept``, the number
	of rows with a finite ``TIME`` per file.  Returns ``(groups, index, moves)``.

	``groups``: a list of ``(shape, bucket, own, files)``: ``shape = (H, W, T)``, ``bucket`` the number of the file's header shape
	(:func:`bucket_files`), ``own`` False for the bucket's regular group -- the files whose ``T`` is the bucket's most common one (of two
	equally common ones the one met first), which stay in the bucket's cubes -- and True for a sub-group of files with another ``T``,
	which gets cubes of its own; ``files[slot]`` is the input number of the file in that slot.  A bucket's regular group comes first, its
	sub-groups follow in the order of their first file.
	``index[i] = (group, slot)`` of input file ``i``.
	``moves``: ``(bucket, source slot, group, slot)`` in the order they have to be made: first every odd file out of its bucket slot
	into its sub-group, then, for every hole this leaves below the number ``n`` of regular files, lowest first, the regular file
	of the highest slot still at or above ``n`` into it.  The regular files then lie in slots ``[0, n)``.
	"""
	keys, members = bucket_files(shapes)
	groups, index, moves = [], [None] * len(shapes), []
	for b, files in enumerate(members):
		H, W, _ = keys[b]
		counts = {}
		for i in files:
			counts[int(kept[i])] = counts.get(int(kept[i]), 0) + 1
		mode = max(counts, key=lambda t: (counts[t], -[int(kept[i]) for i in files].index(t)))
		n = counts[mode]
		slots = list(files)                                              # slots[j]: the file in bucket slot j
		regular = len(groups)
		groups.append(((H, W, mode), b, False, None))
		sub = {}
		for j, i in enumerate(files):
			t = int(kept[i])
			if t == mode:
				continue
			if t not in sub:
				sub[t] = len(groups)
				groups.append(((H, W, t), b, True, []))
			g = sub[t]
			moves.append((b, j, g, len(groups[g][3])))
			groups[g][3].append(i)
			slots[j] = None
		high = len(slots) - 1
		for j in range(n):
			if slots[j] is not None:
				continue
			while slots[high] is None:
				high -= 1
			moves.append((b, high, regular, j))
			slots[j], slots[high] = slots[high], None
		groups[regular] = ((H, W, mode), b, False, slots[:n])
	for g, (_, _, _, files) in enumerate(groups):
		for slot, i in enumerate(files):
			index[i] = (g, slot)
	return groups, index, moves


def load_tpf_groups(ctx, files, verify=True, headers=None):
	"""
	:func:`load_tpfs` for a batched run: the files are unpacked straight into cubes of many targets, one set of three cubes per group of
	files with the same ``(H, W, T)``.  Returns ``(groups, index)``: a list of :class:`TpfGroup` and, per input file in input order, its
	``(group, slot)``.

	Every header is read and checked before anything is allocated, as in :func:`load_tpfs`, and the files are put into buckets by
	``(H, W, NAXIS2)``.  A bucket gets three cubes ``[files][H * W][t_pitch]`` with ``t_pitch`` from ``NAXIS2``; each file streams through
	the same two staging buffers and one ``tp_tpf_unpack`` writes it, pads included, into its slot -- its kept rows ``T`` are known on
	the host before that call is queued.  Once all files are in, :func:`plan_groups` says which files of a bucket have another ``T`` than
	the bucket's most common one: each of them is moved (``tp_memcpy_d2d``) into the cubes of its own sub-group, which keep the bucket's
	``t_pitch``, and a hole it leaves among the regular files is filled from the bucket's last regular slot.  A run without odd files
	moves nothing; an odd file costs one move out and at most one move into its hole.  No pixel passes through host memory and no file
	lies in two cubes.  ``verify``, :class:`ffi.ChecksumError` and the promise that after any exception everything is freed are those of
	:func:`load_tpfs`.  ``headers``: the :class:`TPFHeader` of every file when the caller has read them already.
	"""
	files = [str(f) for f in files]
	if not files:
		raise ValueError("load_tpf_groups: no files")
	infos = [read_tpf_header(f) for f in files] if headers is None else list(headers)
	if len(infos) != len(files):
		raise ValueError("load_tpf_groups: one header per file")
	_check_aperture_units(infos)
	shapes = [h.aperture.shape + (h.table.n_rows,) for h in infos]
	keys, members = bucket_files(shapes)
	slot_of = {i: (b, j) for b, m in enumerate(members) for j, i in enumerate(m)}
	names = [name for name, _ in IMAGE_COLUMNS]
	loaded, owned, buckets, out_groups = [], [], [], []

	def bucket_slot(i, out):
		"""Slot ``j`` of the three cubes of file ``i``'s bucket, their pitch from ``NAXIS2``."""
		b, j = slot_of[i]
		H, W = out.aperture.shape
		pitch = buckets[b][names[0]].t_pitch
		return [buckets[b][name].ptr + j * H * W * pitch * 4 for name in names], pitch
	try:
		for (H, W, n_rows), m in zip(keys, members):
			buckets.append({})
			for name in names:
				cube = DeviceCube(ctx, len(m), n_rows, H, W)
				owned.append(cube)
				buckets[-1][name] = cube
		with _staging(ctx, infos, verify) as st:
			up = st.up
			_stream_files(st, infos, verify, loaded, bucket_slot)
			plan, index, moves = plan_groups(shapes, [len(ld.time) for ld in loaded])
			cubes_of = []
			for (H, W, T), b, own, members_g in plan:
				if own:
					cubes = {name: DeviceCube(ctx, len(members_g), T, H, W, t_pitch=buckets[b][name].t_pitch) for name in names}
					owned.extend(cubes.values())
				else:
					cubes = buckets[b]
				cubes_of.append(cubes)
			if any(own for _, _, own, _ in plan):
				ctx.sync()                                               # the cubes of the sub-groups exist before the other stream writes them
			for b, src, g, slot in moves:
				(H, W, _), _, _, _ = plan[g]
				for name in names:
					one = H * W * buckets[b][name].t_pitch * 4
					up._check(up.lib.tp_memcpy_d2d(up.handle, cubes_of[g][name].ptr + slot * one, buckets[b][name].ptr + src * one, one))
			sums = st.finish()
		if verify:
			for h, got in zip(infos, sums):
				check_datasum(h.path, h.table.hdu, got, h.table.datasum)
		for g, ((H, W, T), b, own, members_g) in enumerate(plan):
			n = len(members_g)
			cubes = {}
			for name in names:
				whole = cubes_of[g][name]
				whole.n_cad = T
				cubes[name] = whole if whole.n_targets == n else whole.slice0(0, n)
			for slot, i in enumerate(members_g):
				loaded[i].cubes = {name: cubes[name].slice0(slot, 1) for name in names}
			out_groups.append(TpfGroup((H, W, T), cubes, [cubes_of[g][name] for name in names], [loaded[i] for i in members_g]))
	except BaseException:
		for cube in owned:
			cube.free()                                                  # (the transfer context has been synced: nothing can write into a cube any more)
		raise
	return out_groups, index


def jitter_lookup(time, timecorr):
	"""
	The row of a file's ``pos_corr`` the plugin applies at cadence ``k``: ``argmin(|tref - tref[k]|)`` with ``tref = time - timecorr``
	(``BasePhotometry.catalog_attime`` for a source with ``jitter``, called with ``tref[k]`` by the LinPSF plugin).  Returns ``None`` when
	that is ``k`` for every cadence, else the int32 vector.  For finite values it is the first cadence with the value of ``tref[k]``
	-- ``k`` itself unless values repeat --, found by sorting; numpy's ``argmin`` returns the first NaN it meets, so with a value that is
	not finite in ``tref`` the rows are computed as the plugin computes them, cadence by cadence (``T^2`` differences, in pieces).
	"""
	tref = np.asarray(time, dtype='float64') - np.asarray(timecorr, dtype='float64')
	T = len(tref)
	if T == 0:
		return None
	if np.all(np.isfinite(tref)):
		if np.all(tref[1:] > tref[:-1]):
			return None
		_, first, inverse = np.unique(tref, return_index=True, return_inverse=True)
		lookup = first[np.asarray(inverse).reshape(-1)]
	else:
		lookup = np.empty(T, dtype='int64')
		step = max(1, (1 << 22) // T)
		with np.errstate(invalid='ignore'):
			for a in range(0, T, step):
				lookup[a:a + step] = np.argmin(np.abs(tref[None, :] - tref[a:a + step, None]), axis=1)
	if np.array_equal(lookup, np.arange(T)):
		return None
	return lookup.astype('int32')


def _needs_projection(d):
	return d is not None and 'row' not in d and 'column' not in d and 'ra' in d and 'dec' in d


def project_for_files(ctx, loaded, catalog, targets=None, max_points=1 << 24):
	"""
	The pixel positions :class:`TpfStampSource` gives a ``catalog`` / ``targets`` in ``ra`` / ``dec`` for every file of ``loaded``, without
	one device call per file: the WCSs of the files' APERTURE headers are the frames of ``tp_wcs_world2pix`` and the points are the
	catalogue as one batch and every target as a batch of its own, which is how the source projects them (``all_world2pix`` with its
	defaults; the stopping test is per batch and frame).  Returns ``(catalog_px, targets_px)``, each ``None`` when that dict needs no
	projection, else float64 ``(files, points, 2)`` of 0-based ``(x, y)`` relative to the stamp: the caller adds the stamp's place on the
	CCD.  At most ``max_points`` positions are formed per call of the entry (``max_points // points`` files, never more than 65 535).
	A point that does not converge raises :class:`photometry_amd.wcs.NoConvergence` naming the file, as the source would.
	"""
	from . import wcs as W
	need_c, need_t = _needs_projection(catalog), _needs_projection(targets)
	if not (need_c or need_t):
		return None, None
	for ld in loaded:
		if not ld.wcs_cards:
			raise ValueError(f"{ld.path}: the catalogue is in ra / dec and the APERTURE header has no WCS to project it through")
	params = W.pack([W.TanSipWCS.from_header(ld.wcs_cards) for ld in loaded])
	empty = np.zeros((0, 2))
	pc = np.column_stack((catalog['ra'], catalog['dec'])).astype('float64') if need_c else empty
	pt = np.column_stack((targets['ra'], targets['dec'])).astype('float64') if need_t else empty
	nc, nt = len(pc), len(pt)
	n = nc + nt
	pts = np.ascontiguousarray(np.concatenate((pc, pt)))
	offsets = np.concatenate(([0], nc + np.arange(nt + 1))).astype('int64')
	d_radec = ctx.array(pts if n else np.zeros((1, 2)))
	d_cos = ctx.empty((max(n, 1), 3), 'float64')
	ctx._check(ctx.lib.tp_wcs_radec(ctx.handle, n, d_radec.ptr, d_cos.ptr))
	F = len(loaded)
	out = np.empty((F, n, 2))
	step = max(1, min(65535, int(max_points) // max(n, 1)))
	for a in range(0, F, step):
		f = min(step, F - a)
		d_params = ctx.array(params[a:a + f])
		pix, status, iters = W.world2pix_frames(ctx, d_params, f, d_cos, n, offsets, 0, 1, 1e-4, 20)
		bad = np.flatnonzero(np.any(status & (W.DIVERGENT | W.SLOW), axis=1))
		if len(bad):
			k = int(bad[0])
			div, slow = np.flatnonzero(status[k] & W.DIVERGENT), np.flatnonzero(status[k] & W.SLOW)
			raise W.NoConvergence(f"{loaded[a + k].path}: 'WCS.all_world2pix' failed to converge to the requested accuracy after {int(iters[k].max()):d} iterations.",
				best_solution=pix[k], divergent=div if len(div) else None, slow_conv=slow if len(slow) else None, niter=int(iters[k].max()))
		out[a:a + f] = pix
	return (out[:, :nc] if need_c else None), (out[:, nc:] if need_t else None)


def main_targets(files, ticids, targets=None):
	"""
	The ``starid`` of the main target of every file of a batched run: the file's ``TICID``, unless ``targets`` has a ``'file'`` column
	with entries that name the file's path -- then the ``j``-th time the path appears in ``files`` it takes the ``starid`` of its
	``j``-th entry (the reference's ``tpf:starid``: a file is listed once per extra target).  ``ValueError`` for a file listed more often
	than it has entries, or without entries and without a ``TICID``.
	"""
	entries = {}
	if targets is not None and 'file' in targets:
		for k, name in enumerate(targets['file']):
			if name is not None and str(name) != '':
				entries.setdefault(str(name), []).append(int(np.asarray(targets['starid'])[k]))
	seen, out = {}, []
	for path, ticid in zip(files, ticids):
		path = str(path)
		if path in entries:
			j = seen.get(path, 0)
			seen[path] = j + 1
			if j >= len(entries[path]):
				raise ValueError(f"{path}: listed {j + 1} times, but targets names it {len(entries[path])} times")
			out.append(entries[path][j])
		elif ticid is None:
			raise ValueError(f"{path}: the primary header has no TICID and targets names no target for the file")
		else:
			out.append(int(ticid))
	return out


def _check_aperture_units(infos):
	for h in infos:
		if h.aperture.bitpix != 32:
			raise ValueError(f"{h.path}: the APERTURE image has BITPIX {h.aperture.bitpix}, not 32")
		for key in ('CRVAL1P', 'CRVAL2P'):
			if key not in h.aperture.header:
				raise ValueError(f"{h.path}: the APERTURE header lacks the {key} card")


def _host_side(h, buf):
	"""Everything of a :class:`LoadedTPF` but its cubes, from the headers ``h`` and the staging buffer ``buf`` that begins at the table."""
	tb, ap = h.table, h.aperture
	out = LoadedTPF()
	out.path = h.path
	out.header = dict(h.header)
	out.sector, out.camera, out.ccd, out.data_rel = (h.header.get(k) for k in ('SECTOR', 'CAMERA', 'CCD', 'DATA_REL'))
	timedel = tb.header.get('TIMEDEL')
	out.cadence = None if timedel is None else int(np.round(timedel * 86400))
	out.readnoise = tb.header.get('READNOIA', 10)
	out.gain = tb.header.get('GAINA', 100)
	out.num_frm = tb.header.get('NUM_FRM', 60)
	out.n_readout = tb.header.get('NREADOUT', 48)
	time = _column_view(buf, tb, 'TIME', 0)
	good = np.isfinite(time)
	out.rows_dropped = int(tb.n_rows - good.sum())
	out._kept_rows = np.flatnonzero(good)
	out.time = time[good].astype('float64')
	out.timecorr = _column_view(buf, tb, 'TIMECORR', 0)[good].astype('float32')
	out.cadenceno = _column_view(buf, tb, 'CADENCENO', 0)[good].astype('int32')
	out.quality = _column_view(buf, tb, 'QUALITY', 0)[good].astype('int32')
	out.pos_corr = np.column_stack((_column_view(buf, tb, 'POS_CORR1', 0)[good], _column_view(buf, tb, 'POS_CORR2', 0)[good])).astype('float64')
	out.time_offset_corrected = False
	if out.data_rel is not None:
		out.time, out.time_offset_corrected = time_offset(out.time, h.header, datatype='tpf', return_flag=True)
	H, W = ap.shape
	out.aperture = np.ndarray((H, W), dtype='>i4', buffer=buf, offset=ap.offset - tb.offset).astype('int32')
	r0, c0 = int(ap.header['CRVAL2P']) - 1, int(ap.header['CRVAL1P']) - 1
	out.max_stamp = (r0, r0 + H, c0, c0 + W)
	out.wcs_cards = ffi.wcs_header_string(ap.cards)
	return out


#--------------------------------------------------------------------------------------------------
class TpfStampSource(MemoryStampSource):
	"""
	A loaded target pixel file as a stamp source of the plugin API: the attributes ``BasePhotometry.__init__`` reads, the whole
	postage stamp as the only frame (``max_stamp``), ``jitter = loaded.pos_corr`` (BasePhotometry.py:471), the primary header with
	``TIME_OFFSET_CORRECTED``, ``aperture_image`` (what ``BasePhotometry.aperture`` crops for a ``tpf`` run) and ``device_cubes``
	(the loader's cubes, which ``AperturePhotometry`` adopts when they live on its own context).  The host frames are filled from
	the cubes on the first ``cutout``.

	``catalog`` / ``targets``: as for :class:`MemoryStampSource`, with ``row`` / ``column`` in CCD pixels; given as ``ra`` / ``dec``
	they are projected through ``wcs`` (default: the WCS of the APERTURE header, which is relative to the stamp) and moved by
	the stamp's place on the CCD (BasePhotometry.py:1159-1165, :461-464).
	"""

	def __init__(self, loaded, catalog, targets=None, wcs=None, prf=None):
		self.loaded = loaded
		r0, _, c0, _ = loaded.max_stamp
		H, W = loaded.aperture.shape
		catalog = dict(catalog)
		targets = None if targets is None else dict(targets)
		if wcs is None and loaded.wcs_cards and (_needs_projection(catalog) or _needs_projection(targets)):
			wcs = loaded.wcs_cards
		if wcs is not None:
			from .wcs import as_wcs
			cube = (loaded.cubes or {}).get('images')
			wcs = as_wcs(wcs, ctx=None if cube is None else cube.ctx)
			if _needs_projection(catalog):
				px = wcs.all_world2pix(np.column_stack((catalog['ra'], catalog['dec'])), 0)
				catalog['column'] = (px[:, 0] + c0).astype('float32')
				catalog['row'] = (px[:, 1] + r0).astype('float32')
			if _needs_projection(targets):
				pos = np.array([wcs.all_world2pix(np.array([[r, d]], dtype='float64'), 0)[0]
					for r, d in zip(np.asarray(targets['ra'], dtype='float64'), np.asarray(targets['dec'], dtype='float64'))]).reshape(-1, 2)
				targets['column'], targets['row'] = pos[:, 0] + c0, pos[:, 1] + r0
		# (the frames are stood in for by a zero-stride view of the stamp's shape until the first cut-out asks for them)
		shape = (H, W, len(loaded.time))
		standin = {name: np.broadcast_to(np.float32(0), shape) for name, _ in IMAGE_COLUMNS}
		super().__init__(standin, r0, c0, loaded.time, loaded.timecorr, loaded.cadenceno, loaded.quality, catalog, sector=loaded.sector,
			camera=loaded.camera, ccd=loaded.ccd, cadence=loaded.cadence, n_readout=loaded.n_readout, jitter=loaded.pos_corr, prf=prf, targets=targets, wcs=wcs)
		self.frames = None
		self.max_stamp = tuple(loaded.max_stamp)
		self.num_frm = loaded.num_frm
		self.header = dict(loaded.header)
		self.header['TIME_OFFSET_CORRECTED'] = bool(loaded.time_offset_corrected)
		self.time_offset_corrected = bool(loaded.time_offset_corrected)
		self.aperture_image = loaded.aperture
		self.device_cubes = loaded.cubes

	def cutout(self, stamp):
		if self.frames is None:
			self.frames = {name: cube.to_host()[0] for name, cube in self.device_cubes.items()}
		return super().cutout(stamp)
