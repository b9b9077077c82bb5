# -*- coding: utf-8 -*-
"""
Synthetic target pixel files and binary tables for the tests of ``photometry_amd.tpf``, written WITHOUT ``photometry_amd.fitsio``:
header cards formatted by hand (tests/ffi_common.py), rows from numpy's big-endian record dtypes, the DATASUM as the word sum modulo
2^32 - 1 -- so that the reader is not held to its own writer.  Image columns travel as ``uint32`` bit patterns, so that signalling
NaNs and payloads reach the file as they were drawn.
"""
import numpy as np
import ffi_common as fc

SENTINEL = 0xDEADBEEF
#: bit patterns planted into random image data: NaN (quiet, signalling, payloads), +-inf, -0.0, 0.0, denormals, 1.0
PLANT = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff8abcde, 0x7fffffff, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001, 0x807fffff, 0x00400000,
	0x3f800000], dtype='uint32')


def random_bits(shape, rng):
	"""Random 32-bit patterns with :data:`PLANT` planted (as many of them as fit)."""
	n = int(np.prod(shape))
	bits = rng.integers(0, 2**32, size=n, dtype='uint64').astype('uint32')
	where = rng.permutation(n)[:len(PLANT)]
	bits[where] = PLANT[:len(where)]
	return bits.reshape(shape)


def round_up(n, m):
	return (int(n) + m - 1) // m * m


# ---- bare tables for the C entry ---------------------------------------------------------------------------------------------------
def bare_table(columns, lead=16, gaps=None, trail=12, rng=None):
	"""
	A binary-table data unit of ``len(columns)`` image columns (uint32 bit patterns ``(n_rows, n_pix)``): every row is ``lead``
	bytes, then the columns with ``gaps[c]`` bytes behind column ``c``, then ``trail`` bytes; what is no column is random.
	Returns ``(bytes, row_bytes, [column offsets])``.
	"""
	rng = rng or np.random.default_rng(0)
	n_rows, n_pix = columns[0].shape
	gaps = list(gaps or [0] * len(columns))
	fields, offsets, pos = [('lead', 'u1', (lead,))], [], lead
	for c, g in enumerate(gaps):
		offsets.append(pos)
		fields += [(f'c{c}', '>u4', (n_pix,)), (f'g{c}', 'u1', (g,))]
		pos += 4 * n_pix + g
	fields.append(('trail', 'u1', (trail,)))
	dt = np.dtype(fields)
	assert dt.itemsize == pos + trail
	rec = np.frombuffer(rng.integers(0, 256, size=n_rows * dt.itemsize, dtype='uint8').tobytes(), dtype=dt).copy()
	for c, col in enumerate(columns):
		rec[f'c{c}'] = col
	return rec.tobytes(), dt.itemsize, offsets


def expected_cube(table, row_bytes, offset, n_pix, rows, t_pitch):
	"""numpy's reading of one image column of the table bytes as a cube ``(n_pix, t_pitch)`` of uint32: the kept rows transposed, then zeros."""
	n_rows = len(table) // row_bytes
	col = np.ndarray((n_rows, n_pix), dtype='>u4', buffer=table, offset=offset, strides=(row_bytes, 4))
	col = col if rows is None else col[np.asarray(rows)]
	out = np.zeros((n_pix, t_pitch), dtype='uint32')
	out[:, :col.shape[0]] = col.astype('uint32').T
	return out


# ---- whole files -------------------------------------------------------------------------------------------------------------------
def pixels_dtype(H, W, image_code='>u4'):
	return np.dtype([('TIME', '>f8'), ('TIMECORR', '>f4'), ('CADENCENO', '>i4'), ('RAW_CNTS', '>i4', (H, W)), ('FLUX', image_code, (H, W)), ('FLUX_ERR', image_code, (H, W)),
		('FLUX_BKG', image_code, (H, W)), ('FLUX_BKG_ERR', '>f4', (H, W)), ('QUALITY', '>i4'), ('POS_CORR1', '>f4'), ('POS_CORR2', '>f4')])


def pixels_cards(H, W, n_rows, image_letter='E', drop=(), tdim=None, extra=()):
	"""The header cards of the PIXELS table (``drop``: column names left out; ``tdim``: per-column override of the TDIM tuple)."""
	n = H * W
	cols = [('TIME', 'D', None), ('TIMECORR', 'E', None), ('CADENCENO', 'J', None), ('RAW_CNTS', f'{n}J', (W, H)), ('FLUX', f'{n}{image_letter}', (W, H)),
		('FLUX_ERR', f'{n}{image_letter}', (W, H)), ('FLUX_BKG', f'{n}{image_letter}', (W, H)), ('FLUX_BKG_ERR', f'{n}E', (W, H)), ('QUALITY', 'J', None),
		('POS_CORR1', 'E', None), ('POS_CORR2', 'E', None)]
	cols = [c for c in cols if c[0] not in drop]
	size = {'D': 8, 'E': 4, 'J': 4}
	row_bytes = sum((int(f[:-1]) if f[:-1] else 1) * size[f[-1]] for _, f, _ in cols)
	cards = [fc.card('XTENSION', 'BINTABLE'), fc.card('BITPIX', 8), fc.card('NAXIS', 2), fc.card('NAXIS1', row_bytes), fc.card('NAXIS2', int(n_rows)), fc.card('PCOUNT', 0),
		fc.card('GCOUNT', 1), fc.card('TFIELDS', len(cols))]
	for i, (name, form, dim) in enumerate(cols, start=1):
		cards += [fc.card(f'TTYPE{i}', name), fc.card(f'TFORM{i}', form)]
		dim = (tdim or {}).get(name, dim)
		if dim is not None:
			cards.append(fc.card(f'TDIM{i}', '(%d,%d)' % tuple(dim)))
	return cards + [fc.card('EXTNAME', 'PIXELS')] + list(extra), row_bytes


def aperture_cards(H, W, crval1p=200, crval2p=300, wcs=True, extra=()):
	cards = fc.image_cards(fc.card('XTENSION', 'IMAGE'), 32, (H, W)) + [fc.card('PCOUNT', 0), fc.card('GCOUNT', 1), fc.card('EXTNAME', 'APERTURE')]
	if wcs:
		cards += [c for c in fc.tan_cards(crpix=((W + 1) / 2, (H + 1) / 2)) if not c.startswith(('CTYPE1P', 'CRPIX1P'))]
	if crval1p is not None:
		cards += [fc.card('WCSNAMEP', 'PHYSICAL'), fc.card('CTYPE1P', 'RAWX'), fc.card('CRPIX1P', 1), fc.card('CRVAL1P', int(crval1p)), fc.card('CTYPE2P', 'RAWY'),
			fc.card('CRPIX2P', 1), fc.card('CRVAL2P', int(crval2p))]
	return cards + list(extra)


PRIMARY = dict(SECTOR=14, CAMERA=2, CCD=3, DATA_REL=35, PROCVER='spoc-5.0.20-20201120', TICID=261136679)


def primary_cards(**values):
	v = dict(PRIMARY)
	v.update(values)
	return [fc.card('SIMPLE', True), fc.card('BITPIX', 8), fc.card('NAXIS', 0), fc.card('EXTEND', True), fc.card('TELESCOP', 'TESS')] + \
		[fc.card(k, x) for k, x in v.items() if x is not None]


def make_tpf(rng, H, W, n_rows, bad_times=(), primary=None, table_extra=None, crval1p=200, crval2p=300, image_code='>u4', image_letter='E', aperture=None, images=None, scalars=None):
	"""
	A whole target pixel file.  Returns ``(blob, rec, aperture, info)``: the bytes, the table as numpy record array (big-endian dtype:
	numpy's own reading of the rows), the int32 APERTURE image, and where the data units lie (counted from the pieces' lengths).
	``images``: dict ``FLUX`` / ``FLUX_ERR`` / ``FLUX_BKG`` of float32 ``(n_rows, H, W)`` instead of random bit patterns; ``scalars``: dict
	of scalar columns instead of the drawn ones; ``bad_times``: rows whose TIME is NaN.
	"""
	dt = pixels_dtype(H, W, image_code)
	rec = np.zeros(n_rows, dtype=dt)
	rec['TIME'] = 1683.35 + np.arange(n_rows) * (120.0 / 86400.0) + rng.normal(size=n_rows) * 1e-7
	rec['TIME'][list(bad_times)] = np.nan
	rec['TIMECORR'] = (3.1e-3 + rng.normal(size=n_rows) * 1e-5).astype('float32')
	rec['CADENCENO'] = 250000 + np.arange(n_rows)
	rec['RAW_CNTS'] = rng.integers(0, 2**20, size=(n_rows, H, W))
	for name in ('FLUX', 'FLUX_ERR', 'FLUX_BKG'):
		if images is not None:
			rec[name] = np.asarray(images[name], dtype='float32').view('uint32') if image_code == '>u4' else images[name]
		elif image_code == '>u4':
			rec[name] = random_bits((n_rows, H, W), rng)
		else:
			rec[name] = rng.normal(size=(n_rows, H, W))
	rec['FLUX_BKG_ERR'] = rng.normal(size=(n_rows, H, W)).astype('float32')
	rec['QUALITY'] = np.where(rng.random(n_rows) < 0.1, 1 << rng.integers(0, 12, size=n_rows), 0)
	rec['POS_CORR1'] = (rng.normal(size=n_rows) * 0.01).astype('float32')
	rec['POS_CORR2'] = (rng.normal(size=n_rows) * 0.01).astype('float32')
	for name, values in (scalars or {}).items():
		rec[name] = values
	if aperture is None:
		aperture = (rng.integers(0, 2, size=(H, W)) * 1 + rng.integers(0, 2, size=(H, W)) * 2 + rng.integers(0, 2, size=(H, W)) * 8 + 64).astype('int32')
	aperture = np.asarray(aperture, dtype='int32')
	tcards, row_bytes = pixels_cards(H, W, n_rows, image_letter=image_letter,
		extra=[fc.card('TIMEDEL', 120.0 / 86400.0)] + list(table_extra if table_extra is not None else [fc.card('READNOIA', 7.5), fc.card('GAINA', 5.25), fc.card('NUM_FRM', 60), fc.card('NREADOUT', 48)]))
	assert row_bytes == dt.itemsize
	h0 = fc.hdu(primary_cards(**(primary or {})), datasum=False)
	theader = fc.header_bytes(tcards + [fc.card('DATASUM', str(fc.ones_sum(rec.tobytes() + b'\0' * (-rec.nbytes % fc.BLOCK))))])
	tdata = rec.tobytes() + b'\0' * (-rec.nbytes % fc.BLOCK)
	aheader = fc.header_bytes(aperture_cards(H, W, crval1p, crval2p))
	adata = aperture.astype('>i4').tobytes()
	blob = h0 + theader + tdata + aheader + adata + b'\0' * (-len(adata) % fc.BLOCK)
	info = {'table_offset': len(h0) + len(theader), 'table_bytes': len(tdata), 'row_bytes': row_bytes, 'aperture_offset': len(h0) + len(theader) + len(tdata) + len(aheader),
		'aperture_bytes': round_up(len(adata), fc.BLOCK), 'datasum': fc.ones_sum(tdata), 'columns': {n: dt.fields[n][1] for n in dt.names}}
	return blob, rec, aperture, info


def host_cube(rec, name, good=None):
	"""numpy's ``(H, W, T)`` reading of an image column of the record array, as uint32 (the kept rows only)."""
	col = rec[name] if good is None else rec[name][good]
	return np.moveaxis(col.astype('uint32') if col.dtype.kind == 'u' else col.astype('float32').view('uint32'), 0, 2)
