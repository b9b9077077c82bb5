# -*- coding: utf-8 -*-
"""
A binary table's header from its cards and a known DATASUM, without the data (``fitsio.bintable_header``), and the light-curve file in
pieces around a table formed elsewhere (``lcfile.lightcurve_pieces``): both give, byte for byte, what ``fitsio.bintable_hdu`` and
``lcfile.lightcurve_hdus`` give.  No GPU.
"""
import numpy as np
import pytest
from photometry_amd import fitsio, lcfile

T, H, W = 40, 5, 6
STAMP = (100, 105, 200, 206)


def _columns(n, seed=0):
	rng = np.random.default_rng(seed)
	arrays = {'TIME': 1700.0 + np.arange(n) / 48, 'TIMECORR': rng.normal(size=n) * 1e-3, 'CADENCENO': np.arange(n, dtype='int32') + 4700, 'FLUX_RAW': rng.normal(1e4, 10, n),
		'FLUX_RAW_ERR': rng.uniform(1, 2, n), 'FLUX_BKG': rng.normal(100, 1, n), 'FLUX_CORR': np.full(n, np.nan), 'FLUX_CORR_ERR': np.full(n, np.nan),
		'QUALITY': rng.integers(0, 512, n).astype('int32'), 'PIXEL_QUALITY': rng.integers(0, 64, n).astype('int32'), 'MOM_CENTR1': rng.normal(size=n) + 203.0,
		'MOM_CENTR2': rng.normal(size=n) + 102.0, 'POS_CORR1': rng.normal(size=n) * 0.01, 'POS_CORR2': rng.normal(size=n) * 0.01}
	return [dict(c, array=arrays[c['name']]) for c in lcfile.table_columns()]


def _without_arrays(columns):
	return [{k: v for k, v in c.items() if k != 'array'} for c in columns]


@pytest.mark.parametrize('n', [0, 1, 31])
def test_header_plus_data_is_the_hdu(n):
	columns = _columns(n, seed=n)
	cards = [fitsio.card('INHERIT', True, 'inherit the primary header'), fitsio.card('TSTART', 1699.5, 'observation start time in BTJD')]
	hdu = fitsio.bintable_hdu('LIGHTCURVE', columns, cards)
	data = fitsio.bintable_data(columns)
	assert len(data) == fitsio._padded(96 * n) and hdu.endswith(data)
	header = fitsio.bintable_header('LIGHTCURVE', _without_arrays(columns), cards, n, fitsio._sum32(data) if data else 0)
	assert len(header) % fitsio.BLOCK == 0 and header + data == hdu
	# another datasum gives other DATASUM and CHECKSUM cards, and nothing else
	other = fitsio.bintable_header('LIGHTCURVE', _without_arrays(columns), cards, n, 12345)
	differ = [k for k in range(0, len(header), 80) if header[k:k + 80] != other[k:k + 80]]
	assert [header[k:k + 8] for k in differ] == [b'CHECKSUM', b'DATASUM ']


def test_the_14_columns_are_96_bytes():
	columns = lcfile.table_columns()
	assert [c['format'] for c in columns] == list('DEJDDDDDJJDDDD') and all('array' not in c for c in columns)
	assert fitsio._bintable_dtype(columns).itemsize == 96
	assert [c['name'] for c in columns] == ['TIME', 'TIMECORR', 'CADENCENO', 'FLUX_RAW', 'FLUX_RAW_ERR', 'FLUX_BKG', 'FLUX_CORR', 'FLUX_CORR_ERR', 'QUALITY',
		'PIXEL_QUALITY', 'MOM_CENTR1', 'MOM_CENTR2', 'POS_CORR1', 'POS_CORR2']


def _weightmap():
	rng = np.random.default_rng(3)
	return {'weightmap': rng.random((2, H, W)).astype('float32'), 'initial_cadence': np.array([4700, 4706]), 'final_cadence': np.array([4705, 4711]),
		'sat_pixels': np.array([3, 4])}


def test_weightmap_shaped_table_with_a_tdim():
	wm = _weightmap()
	icards = [fitsio.card('STAMP_R1', 100), fitsio.card('INHERIT', True, 'inherit the primary header')]
	hdu = lcfile.weightmap_hdu(wm, (H, W), icards)
	columns = [
		{'name': 'CADENCENO1', 'format': 'J', 'array': np.asarray(wm['initial_cadence'], dtype='int32'), 'disp': 'I10', 'comments': {'TTYPE': 'first'}},
		{'name': 'SAT_PIXELS', 'format': 'J', 'array': np.asarray(wm['sat_pixels'], dtype='int32'), 'disp': 'I10'},
		{'name': 'WEIGHTMAP', 'format': f'{H * W}E', 'array': wm['weightmap'], 'disp': 'E14.7', 'dim': (W, H), 'comments': {'TDIM': 'column dimensions: pixel aperture array'}},
	]
	full = fitsio.bintable_hdu('WEIGHTMAP', columns, icards)
	data = fitsio.bintable_data(columns)
	assert len(data) == fitsio.BLOCK and b'TDIM3' in full
	assert fitsio.bintable_header('WEIGHTMAP', _without_arrays(columns), icards, 2, fitsio._sum32(data)) + data == full
	# the file's own WEIGHTMAP table ends with a data unit of the same size (four columns: 16 + 4 * H * W bytes per row)
	assert len(hdu) % fitsio.BLOCK == 0 and fitsio._padded(2 * (16 + 4 * H * W)) == fitsio.BLOCK


def _lightcurve(time):
	rng = np.random.default_rng(1)
	n = len(time)
	return {'time': np.asarray(time, dtype='float64'), 'timecorr': rng.normal(size=n) * 1e-3, 'cadenceno': np.arange(n, dtype='int32') + 4700,
		'quality': (np.arange(n) % 3 == 0).astype('int32') * 32, 'flux': rng.normal(1e4, 10, n), 'flux_err': rng.uniform(1, 2, n),
		'flux_background': rng.normal(100, 1, n), 'pos_centroid': rng.normal(size=(n, 2)) + (203.0, 102.0), 'pos_corr': rng.normal(size=(n, 2)) * 0.01}


def _images():
	rng = np.random.default_rng(2)
	sumimage = rng.uniform(10, 1e4, (H, W))
	sumimage[0, 0] = np.nan
	mask = np.zeros((H, W), dtype=bool)
	mask[1:4, 2:5] = True
	return sumimage, lcfile.aperture_with_masks(lcfile.ffi_aperture(sumimage, STAMP), mask, mask)


@pytest.mark.parametrize('method,drop', [('aperture', ()), ('aperture', (0, 17, T - 1)), ('halo', ()), ('halo', (5,)), ('aperture', tuple(range(T)))])
def test_pieces_around_the_host_data_unit_are_the_file(method, drop):
	time = 1700.0 + np.arange(T) / 48
	time[list(drop)] = np.nan
	lc = _lightcurve(time)
	quality = (np.arange(T, dtype='int32') % 5) * 256
	sumimage, aperture = _images()
	weightmap = _weightmap() if method == 'halo' else None
	headers = {'HALO_VER': ('x-1', 'Version of halo photometry')} if method == 'halo' else {'AP_CONT': (0.0125, 'AP contamination'), 'KP_WS': (True, 'K2P2 watershed segmentation')}
	args = ({'tmag': 9.25, 'ra_J2000': 290.5, 'pm_ra': 3.0, 'pm_decl': 4.0}, 261136679, 14, 2, 3, 1800, 20, 6, method, 8, {'CRMITEN': True, 'CRBLKSZ': 10, 'CRSPOC': False, 'DATA_REL': 20},
		900, 720, headers)
	hdus = lcfile.lightcurve_hdus(*args, lc, quality, sumimage, aperture, lcfile.image_cards(STAMP), weightmap=weightmap)
	assert len(hdus) == (5 if method == 'halo' else 4)
	pieces = lcfile.lightcurve_pieces(*args, time, sumimage, aperture, lcfile.image_cards(STAMP), weightmap=weightmap)
	assert pieces.rows.dtype == np.dtype('int32') and np.array_equal(pieces.rows, np.flatnonzero(np.isfinite(time)))
	n = len(pieces.rows)
	data = hdus[1][len(hdus[1]) - fitsio._padded(96 * n):] if n else b''
	header = fitsio.bintable_header('LIGHTCURVE', pieces.columns, pieces.cards, n, fitsio._sum32(data) if data else 0)
	assert pieces.front == hdus[0] and header + data == hdus[1] and pieces.back == b''.join(hdus[2:])
	assert pieces.front + header + data + pieces.back == b''.join(hdus)
