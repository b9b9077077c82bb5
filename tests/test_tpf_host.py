# -*- coding: utf-8 -*-
"""
CPU checks of the target-pixel-file input path: the host side of ``photometry_amd.tpf`` (``find_tpf_files``, ``read_tpf_header``,
``time_offset``) on files written by tests/tpf_common.py, and the device-free rules of the unpacker (photometry_amd/csrc/tpf_rules.h)
compiled for the host with AddressSanitizer and UBSan into tests/hostsim/tpf_rules_host.cpp, whose serial composition of the rules
into a complete unpack is held to numpy's reading of the same bytes, bit for bit.
"""
import os
import re
import subprocess
import numpy as np
import pytest
import conftest
import ffi_common as fc
import tpf_common as tc
from photometry_amd import tpf

CSRC = os.path.join(conftest.ROOT, 'photometry_amd', 'csrc')
SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'tpf_rules_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'tpf_rules_host')


# ---- find_tpf_files ----------------------------------------------------------------------------------------------------------------
def test_find_tpf_files(tmp_path):
	names = {                                                                            # (starid, sector, cadence)
		'a/tess2019199201929-s0014-0000000261136679-0150-s_tp.fits': (261136679, 14, 120),
		'b/tess2019199201929-s0014-0000000261136679-0150-a_fast-tp.fits': (261136679, 14, 20),
		'tess2019226182529-s0015-0000000261136679-0151-s_tp.fits.gz': (261136679, 15, 120),
		'c/d/tess2019199201929-s0014-0000000025155310-0150-s_tp.fits': (25155310, 14, 120),
		'hlsp_tess-data-alerts_tess_phot_00261136679-s14_tess_v1_tp.fits': (261136679, 14, 120),
		'hlsp_tess-data-alerts_tess_phot_00025155310-s02_tess_v1_tp.fits.gz': (25155310, 2, 120),
		'tess2019199201929-s0014-0000000261136679-0150-s_lc.fits': None,                   # a light curve
		'tess2019199201929-s014-0000000261136679-0150-s_tp.fits': None,                    # three-digit sector
		'tess2019199201929-s0014-0000000261136679-0150-q_tp.fits': None,
		'tess2019199201929-s0014-0000000261136679-0150-s_tp.fits.bak': None,
		'hlsp_tess-data-alerts_tess_phot_00261136679-s014_tess_v1_tp.fits': None,          # three-digit sector of the alert pattern
		'tess2019199201929-s0014-1-1-0150-s_ffic.fits': None,
	}
	for n in names:
		os.makedirs(tmp_path / os.path.dirname(n), exist_ok=True)
		(tmp_path / n).write_bytes(b'')

	def want(starid=None, sector=None, cadence=None):
		keep = [n for n, v in names.items() if v and (starid is None or v[0] == starid) and (sector is None or v[1] == sector) and (cadence is None or v[2] == cadence)]
		return [str(tmp_path / n) for n in sorted(keep, key=os.path.basename)]
	root = str(tmp_path)
	every = tpf.find_tpf_files(root)
	assert every == want() and len(every) == 6
	assert [os.path.basename(f) for f in every] == sorted(os.path.basename(f) for f in every)
	assert tpf.find_tpf_files(root, cadence=120) == want(cadence=120) and len(want(cadence=120)) == 5          # tp, not fast-tp; alerts are 120 s
	assert tpf.find_tpf_files(root, cadence=20) == want(cadence=20) and len(want(cadence=20)) == 1              # fast-tp alone, no alert files
	assert tpf.find_tpf_files(root, sector=14) == want(sector=14) and len(want(sector=14)) == 4                 # 4-digit and the alert's 2-digit
	assert tpf.find_tpf_files(root, sector=2) == want(sector=2) and len(want(sector=2)) == 1
	assert tpf.find_tpf_files(root, sector=15, cadence=20) == []
	# one star: its files sorted by base name
	mine = tpf.find_tpf_files(root, starid=261136679)
	assert mine == want(starid=261136679) and len(mine) == 4
	assert [os.path.basename(f)[:4] for f in mine] == ['hlsp', 'tess', 'tess', 'tess']
	assert tpf.find_tpf_files(root, starid=25155310, sector=14) == want(25155310, 14)
	assert tpf.find_tpf_files(root, starid=1) == []
	assert tpf.find_tpf_files(root, findmax=2) == every[:2]
	assert tpf.find_tpf_files(root, starid=261136679, findmax=1) == mine[:1]
	for bad in (30, 1800, 0):
		with pytest.raises(ValueError, match='cadence'):
			tpf.find_tpf_files(root, cadence=bad)
	# not cached: a new file is seen
	(tmp_path / 'tess2019226182529-s0015-0000000000000007-0151-s_tp.fits').write_bytes(b'')
	assert len(tpf.find_tpf_files(root)) == 7


def test_find_tpf_files_by_camera_and_ccd_reads_the_primary_header_only(tmp_path):
	place = {'tess2019199201929-s0014-0000000000000001-0150-s_tp.fits': (1, 1), 'tess2019199201929-s0014-0000000000000002-0150-s_tp.fits': (1, 2),
		'tess2019199201929-s0014-0000000000000003-0150-s_tp.fits.gz': (2, 2), 'tess2019199201929-s0014-0000000000000004-0150-s_tp.fits': (2, 2),
		'tess2019199201929-s0014-0000000000000005-0150-s_fast-tp.fits': (2, 2)}
	for n, (camera, ccd) in place.items():
		fc.write(tmp_path / n, fc.header_bytes(tc.primary_cards(CAMERA=camera, CCD=ccd)))           # a primary header and nothing behind it
	root = str(tmp_path)
	base = lambda files: [str(int(re.search(r'-(\d{16})-', os.path.basename(f)).group(1))) for f in files] # noqa: E731
	assert base(tpf.find_tpf_files(root)) == ['1', '2', '3', '4', '5']
	assert base(tpf.find_tpf_files(root, camera=1)) == ['1', '2']
	assert base(tpf.find_tpf_files(root, ccd=2)) == ['2', '3', '4', '5']
	assert base(tpf.find_tpf_files(root, camera=2, ccd=2)) == ['3', '4', '5']
	assert base(tpf.find_tpf_files(root, camera=2, ccd=2, cadence=120)) == ['3', '4']
	assert base(tpf.find_tpf_files(root, camera=2, ccd=2, findmax=2)) == ['3', '4']
	assert base(tpf.find_tpf_files(root, camera=2, ccd=1)) == []
	assert base(tpf.find_tpf_files(root, starid=3, camera=2)) == ['3']


# ---- read_tpf_header ---------------------------------------------------------------------------------------------------------------
def _headers_only(tmp_path, name, H=11, W=12, n_rows=19000, table=None, acards=None):
	"""A TPF cut short behind the APERTURE header: a sparse file, its data units never written.  ``table``: what ``tc.pixels_cards`` returned."""
	h0 = fc.header_bytes(tc.primary_cards())
	cards, row_bytes = table or tc.pixels_cards(H, W, n_rows, extra=[fc.card('TIMEDEL', 120.0 / 86400.0), fc.card('DATASUM', '4242')])
	h1 = fc.header_bytes(cards)
	h2 = fc.header_bytes(tc.aperture_cards(H, W) if acards is None else acards)
	unit = tc.round_up(row_bytes * n_rows, 2880)
	path = tmp_path / name
	with open(path, 'wb') as fh:
		fh.write(h0 + h1)
		fh.seek(len(h0) + len(h1) + unit)
		fh.write(h2)
	return str(path), len(h0), len(h1), len(h2), unit, row_bytes


def test_layout_and_offsets_of_a_file_without_its_data_units(tmp_path):
	path, n0, n1, n2, unit, row_bytes = _headers_only(tmp_path, 't_tp.fits')
	assert os.path.getsize(path) == n0 + n1 + unit + n2                # the APERTURE image is not there at all
	assert row_bytes == 2668 and row_bytes % 16 == 12                  # an 11 x 12 stamp: rows that are only 4-byte aligned
	h = tpf.read_tpf_header(path)
	assert h.header['SECTOR'] == 14 and h.header['CAMERA'] == 2 and h.header['CCD'] == 3 and h.header['DATA_REL'] == 35 and h.header['PROCVER'] == 'spoc-5.0.20-20201120'
	t = h.table
	assert (t.hdu, t.offset, t.nbytes, t.row_bytes, t.n_rows, t.datasum) == (1, n0 + n1, unit, 2668, 19000, 4242)
	assert unit == 50693760 and unit % 2880 == 0
	assert t.header['EXTNAME'] == 'PIXELS' and t.header['TIMEDEL'] == 120.0 / 86400.0
	n = 11 * 12
	want = [('TIME', 'D', 0, None), ('TIMECORR', 'E', 8, None), ('CADENCENO', 'J', 12, None), ('RAW_CNTS', f'{n}J', 16, (12, 11)), ('FLUX', f'{n}E', 16 + 4 * n, (12, 11)),
		('FLUX_ERR', f'{n}E', 16 + 8 * n, (12, 11)), ('FLUX_BKG', f'{n}E', 16 + 12 * n, (12, 11)), ('FLUX_BKG_ERR', f'{n}E', 16 + 16 * n, (12, 11)),
		('QUALITY', 'J', 16 + 20 * n, None), ('POS_CORR1', 'E', 20 + 20 * n, None), ('POS_CORR2', 'E', 24 + 20 * n, None)]
	assert [tuple(c) for c in t.columns.values()] == want and list(t.columns) == [w[0] for w in want]
	a = h.aperture
	assert (a.hdu, a.offset, a.nbytes, a.bitpix, a.shape) == (2, n0 + n1 + unit + n2, 2880, 32, (11, 12))
	assert a.header['CRVAL1P'] == 200 and a.header['CRVAL2P'] == 300 and a.header['EXTNAME'] == 'APERTURE'
	assert len(a.cards) % 80 == 0 and 'CRVAL1P' in a.cards and 'CTYPE1' in a.cards


def test_gz_header_equals_plain_header(tmp_path):
	blob, rec, ap, info = tc.make_tpf(np.random.default_rng(2), 9, 13, 40)
	a = tpf.read_tpf_header(fc.write(tmp_path / 'a_tp.fits', blob))
	b = tpf.read_tpf_header(fc.write(tmp_path / 'a_tp.fits.gz', blob))
	assert a[1:] == b[1:]
	assert a.table.offset == info['table_offset'] and a.table.nbytes == info['table_bytes'] and a.table.datasum == info['datasum']
	assert a.aperture.offset == info['aperture_offset'] and a.aperture.nbytes == info['aperture_bytes']
	assert {n: c.offset for n, c in a.table.columns.items()} == info['columns']
	with pytest.raises(ValueError, match='a_cut'):
		tpf.read_tpf_header(fc.write(tmp_path / 'a_cut_tp.fits', blob[:info['table_offset']]))       # primary HDU and table header alone


@pytest.mark.parametrize('column', ['TIME', 'TIMECORR', 'CADENCENO', 'FLUX', 'FLUX_ERR', 'FLUX_BKG', 'QUALITY', 'POS_CORR1', 'POS_CORR2'])
def test_a_missing_column_is_refused(tmp_path, column):
	path, *_ = _headers_only(tmp_path, f'no_{column}_tp.fits', W=11, n_rows=70, table=tc.pixels_cards(11, 11, 70, drop=(column,)))
	with pytest.raises(ValueError, match=column) as e:
		tpf.read_tpf_header(path)
	assert os.path.basename(path) in str(e.value)


def test_other_refusals_name_the_file_and_the_column(tmp_path):
	# an image column that is not E
	path, *_ = _headers_only(tmp_path, 'double_tp.fits', W=11, n_rows=70, table=tc.pixels_cards(11, 11, 70, image_letter='D'))
	with pytest.raises(ValueError, match=r"double_tp\.fits: image column FLUX has the TFORM '121D'"):
		tpf.read_tpf_header(path)
	# the three image columns differ in TDIM
	path, *_ = _headers_only(tmp_path, 'tdim_tp.fits', W=11, n_rows=70, table=tc.pixels_cards(11, 11, 70, tdim={'FLUX_BKG': (121, 1)}))
	with pytest.raises(ValueError, match=r'tdim_tp\.fits: image column FLUX_BKG has the TDIM \(121, 1\)'):
		tpf.read_tpf_header(path)
	# TDIM disagrees with the APERTURE image
	path, *_ = _headers_only(tmp_path, 'shape_tp.fits', H=11, W=12, n_rows=70, acards=tc.aperture_cards(12, 11))
	with pytest.raises(ValueError, match=r'shape_tp\.fits: .*APERTURE image is 11 x 12'):
		tpf.read_tpf_header(path)
	# a file that is no TPF at all
	img = np.zeros((20, 24), dtype='float32')
	with pytest.raises(ValueError, match='plain'):
		tpf.read_tpf_header(fc.write(tmp_path / 'plain.fits', fc.plain_file(img, img) + fc.plain_file(img, img)))


# ---- time_offset ---------------------------------------------------------------------------------------------------------------
FIRST_27 = ('spoc-4.0.14-20200108', 'spoc-4.0.15-20200114', 'spoc-4.0.17-20200130')
FIRST_29 = ('spoc-4.0.17-20200130', 'spoc-4.0.20-20200220', 'spoc-4.0.21-20200227')
LATER = 'spoc-4.0.26-20200323'


def test_time_offset_by_hand():
	t = np.array([1500.0, 1500.5, 1527.25])
	mid, start, end = (-2.000 + 0.021) / 86400, (-2.000 + 0.031) / 86400, (-2.000 + 0.011) / 86400
	def shift(header, **kw):
		out, flag = tpf.time_offset(t, header, return_flag=True, **kw)
		assert flag == (not np.array_equal(out, t))
		return out - t
	same = np.zeros(3)
	for rel in (1, 20, 26):
		assert np.array_equal(shift({'DATA_REL': rel}), (t + mid) - t)
		assert np.array_equal(tpf.time_offset(t, {'DATA_REL': rel}), t + (-2.000 + 0.021) / 86400)
	for procver in FIRST_27:
		assert np.array_equal(shift({'DATA_REL': 27, 'PROCVER': procver}), (t + mid) - t)
	assert np.array_equal(shift({'DATA_REL': 27, 'PROCVER': LATER}), same)
	assert np.array_equal(shift({'DATA_REL': 27, 'PROCVER': FIRST_29[1]}), same)          # a first release of 29 is none of 27
	for procver in FIRST_29:
		assert np.array_equal(shift({'DATA_REL': 29, 'PROCVER': procver}), (t + mid) - t)
	assert np.array_equal(shift({'DATA_REL': 29, 'PROCVER': LATER}), same)
	assert np.array_equal(shift({'DATA_REL': 29, 'PROCVER': FIRST_27[0]}), same)
	for rel in (27, 29):
		with pytest.raises(ValueError, match='PROCVER'):
			tpf.time_offset(t, {'DATA_REL': rel})
	assert np.array_equal(shift({'DATA_REL': 28}), same)                                  # neither early nor one of the two: no PROCVER needed
	for rel in (30, 35, 60):
		assert np.array_equal(shift({'DATA_REL': rel}), same)
	# already corrected
	assert np.array_equal(shift({'DATA_REL': 20, 'TIME_OFFSET_CORRECTED': True}), same)
	assert np.array_equal(shift({'DATA_REL': 27, 'TIME_OFFSET_CORRECTED': True}), same)     # (without PROCVER: no error either)
	assert np.array_equal(shift({'DATA_REL': 20, 'TIME_OFFSET_CORRECTED': False}), (t + mid) - t)
	# the three positions in the exposure
	assert np.array_equal(shift({'DATA_REL': 20}, timepos='mid'), (t + mid) - t)
	assert np.array_equal(shift({'DATA_REL': 20}, timepos='start'), (t + start) - t)
	assert np.array_equal(shift({'DATA_REL': 20}, timepos='end'), (t + end) - t)
	assert abs(mid * 86400 + 1.979) < 1e-12 and abs(start * 86400 + 1.969) < 1e-12 and abs(end * 86400 + 1.989) < 1e-12
	with pytest.raises(ValueError, match='TIMEPOS'):
		tpf.time_offset(t, {'DATA_REL': 20}, timepos='middle')
	# the staggered readout is an FFI matter: a TPF header with CAMERA and CCD moves by the same amount, an FFI by more
	hdr = {'DATA_REL': 20, 'CAMERA': 2, 'CCD': 3}
	assert np.array_equal(shift(hdr, datatype='tpf'), (t + mid) - t)
	assert np.array_equal(tpf.time_offset(t, hdr, datatype='ffi'), t + (1.500 + 0.040 - 2.000 + 0.021) / 86400)
	assert np.array_equal(tpf.time_offset(t, {'DATA_REL': 27, 'PROCVER': FIRST_27[0], 'CAMERA': 4, 'CCD': 1}, datatype='ffi'), t + (1.000 - 2.000 + 0.021) / 86400)
	assert np.array_equal(tpf.time_offset(t, {'DATA_REL': 29, 'PROCVER': FIRST_29[0], 'CAMERA': 4, 'CCD': 4}, datatype='ffi'), t + (-2.000 + 0.021) / 86400)
	assert tpf.time_offset(t, {'DATA_REL': 35}) is t                                       # nothing to do: the very array comes back


def test_time_offset_settings_switch(tmp_path, monkeypatch, caplog):
	"""``[fixes] time_offset`` of the settings file the package reads (``plugins.load_settings``)."""
	t = np.array([1500.0, 1501.0])
	ini = tmp_path / 'settings.ini'
	ini.write_text('[fixes]\ntime_offset = no\n')
	monkeypatch.setenv('TESSPHOT_SETTINGS', str(ini))
	with caplog.at_level('WARNING', logger='photometry_amd.tpf'):
		out, flag = tpf.time_offset(t, {'DATA_REL': 20}, return_flag=True)
	assert flag is False and np.array_equal(out, t) and 'turned off in settings' in caplog.text
	assert tpf.time_offset(t, {'DATA_REL': 35}, return_flag=True)[1] is False
	ini.write_text('[fixes]\ntime_offset = true\n')
	assert tpf.time_offset(t, {'DATA_REL': 20}, return_flag=True)[1] is True
	monkeypatch.delenv('TESSPHOT_SETTINGS')
	assert tpf.time_offset(t, {'DATA_REL': 20}, return_flag=True)[1] is True                # the default: on


# ---- tpf_rules.h -------------------------------------------------------------------------------------------------------------------
def test_header_compiles_alone(tmp_path):
	src = tmp_path / 'only.cpp'
	src.write_text('#include "tpf_rules.h"\nint main() { return tp_tpf::lds_index(1, 0) - 65; }\n')
	subprocess.run(['g++', '-std=c++17', '-Wall', '-fsyntax-only', '-I' + CSRC, str(src)], check=True)


@pytest.fixture(scope='module')
def driver():
	os.makedirs(OUT_DIR, exist_ok=True)
	subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall', '-I' + CSRC, '-o', OUT, SRC],
		check=True)

	def run(text):
		r = subprocess.run([OUT], input=text, capture_output=True, text=True, timeout=300)
		assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
		assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
		assert r.stderr == '', r.stderr
		assert 'FAILED:' not in r.stdout, r.stdout[-2000:]
		return r.stdout.splitlines()
	return run


def test_tile_maps_cover_a_tile_exactly_once(driver):
	assert driver('maps 1') == ['ok']


A, B = 0x7f0000000100, 0x7f0000800000
#: a good call: table_addr row_bytes n_rows T n_cols offsets n_pix outs t_pitch rows
GOOD = dict(table=A, row_bytes=2448, n_rows=70, T=70, n_cols=3, offs=(500, 984, 1468, 0), n_pix=121, outs=(B, B + 0x10000, B + 0x20000, 0), t_pitch=96, rows=None)


def _check_line(**kw):
	c = dict(GOOD)
	c.update(kw)
	rows = c['rows']
	return ' '.join(['%x' % c['table'], str(c['row_bytes']), str(c['n_rows']), str(c['T']), str(c['n_cols'])] + [str(o) for o in c['offs']] + [str(c['n_pix'])] +
		['%x' % o for o in c['outs']] + [str(c['t_pitch']), str(-1 if rows is None else len(rows))] + [str(r) for r in (rows or [])])


#: every refusal of the issue with a fragment of its message; the same list drives the device test (tests/test_gpu_tpf_unpack.py)
REFUSALS = [
	(dict(table=0), 'null pointer'), (dict(outs=(B, 0, B, 0)), 'null pointer'), (dict(n_cols=-1), 'null pointer'), (dict(n_cols=-2), 'null pointer'),
	(dict(table=A + 2), 'd_table must be 4-byte aligned'), (dict(table=A + 1), '4-byte aligned'),
	(dict(row_bytes=2450), 'row_bytes'), (dict(row_bytes=0), 'row_bytes'), (dict(row_bytes=-2448), 'row_bytes'),
	(dict(offs=(500, 986, 1468, 0)), 'column offset'), (dict(offs=(-4, 984, 1468, 0)), 'column offset'),
	(dict(offs=(500, 984, 1968, 0)), 'leaves the row'), (dict(offs=(500, 984, 2448, 0)), 'leaves the row'), (dict(n_pix=613), 'leaves the row'),
	(dict(n_cols=0), 'n_cols'), (dict(n_cols=5), 'n_cols'),
	(dict(T=0), 'T must lie'), (dict(T=71), 'T must lie'), (dict(T=-1), 'T must lie'), (dict(T=69), 'T must equal n_rows'),
	(dict(t_pitch=64), 't_pitch'), (dict(t_pitch=70), 't_pitch'), (dict(t_pitch=100), 't_pitch'),
	(dict(n_rows=2**34 // 2448 + 1, T=1, rows=[0]), '2^34'), (dict(n_rows=0), 'n_rows'), (dict(n_pix=0), 'n_pix'),
	(dict(T=3, rows=[0, 2, 2]), 'increase strictly'), (dict(T=3, rows=[0, 2, 1]), 'increase strictly'), (dict(T=3, rows=[5, 6, 70]), 'outside the table'),
	(dict(T=3, rows=[-1, 6, 7]), 'outside the table'), (dict(T=2, rows=[69, 68]), 'increase strictly'),
]
ACCEPTED = [dict(), dict(n_cols=1), dict(n_cols=4, offs=(500, 984, 1468, 16), outs=(B, B + 4, B + 8, B + 12)), dict(table=A + 4), dict(offs=(500, 984, 1964, 0)),
	dict(T=3, rows=[0, 68, 69], t_pitch=32), dict(T=70, rows=list(range(70))), dict(t_pitch=128), dict(n_rows=2**34 // 2448, T=1, rows=[2**34 // 2448 - 1], t_pitch=32),
	dict(n_pix=1, offs=(2444, 0, 4, 0))]


def test_every_refusal_returns_its_message(driver):
	out = driver(f'check {len(REFUSALS) + len(ACCEPTED)}\n' + '\n'.join(_check_line(**kw) for kw, _ in REFUSALS) + '\n' + '\n'.join(_check_line(**kw) for kw in ACCEPTED))
	for line, (kw, fragment) in zip(out, REFUSALS):
		assert line.startswith('refused tp_tpf_unpack: ') and fragment in line, (kw, line)
	assert out[len(REFUSALS):] == ['ok'] * len(ACCEPTED), list(zip(ACCEPTED, out[len(REFUSALS):]))


#: (n_pix, n_rows, kept rows or None, what): the shapes of tests/test_gpu_tpf_unpack.py
def _drop(n_rows, gone):
	return [r for r in range(n_rows) if r not in gone]


SHAPES = [(1, 1, None, 'smallest'), (3, 5, None, 'odd'), (64, 64, None, 'one full tile'), (65, 65, None, 'one past a tile both ways'),
	(121, 70, None, 'pads 70..95'), (132, 33, None, 'rows of 12 mod 16 bytes'), (121, 200, _drop(200, (0, 99, 100, 199)), 'rows dropped'),
	(625, 130, _drop(130, (64,)), 'one row dropped, ten pixel tiles'), (121, 19000, None, 'the realistic size')]


@pytest.mark.parametrize('n_pix,n_rows,rows,what', SHAPES, ids=[s[3] for s in SHAPES])
def test_serial_composition_of_the_rules_equals_numpy(driver, tmp_path, n_pix, n_rows, rows, what):
	rng = np.random.default_rng(n_pix + n_rows)
	cols = [tc.random_bits((n_rows, n_pix), rng) for _ in range(3)]
	table, row_bytes, offsets = tc.bare_table(cols, lead=16, gaps=(0, 4, 0), trail=8, rng=rng)
	if n_pix == 132:
		assert row_bytes % 16 == 12
	T = n_rows if rows is None else len(rows)
	t_pitch = tc.round_up(T, 32)
	(tmp_path / 'table.bin').write_bytes(table)
	line = ' '.join(map(str, ['unpack 1', tmp_path / 'table.bin', tmp_path / 'out.bin', row_bytes, n_rows, T, 3] + offsets + [0, n_pix, t_pitch, -1 if rows is None else len(rows)] + (rows or [])))
	out = driver(line)
	# every output element of every tile written exactly once, pads included
	assert out == [f'ok writes {3 * n_pix * t_pitch} min 1 max 1'], out
	got = np.fromfile(tmp_path / 'out.bin', dtype='uint32').reshape(3, n_pix, t_pitch)
	for c in range(3):
		want = tc.expected_cube(table, row_bytes, offsets[c], n_pix, rows, t_pitch)
		assert np.array_equal(got[c], want), (what, c)
		assert np.all(got[c][:, T:] == 0)
	if n_pix == 121 and n_rows == 70:
		assert t_pitch == 96


def test_serial_composition_refuses_like_the_check(driver, tmp_path):
	rng = np.random.default_rng(4)
	table, row_bytes, offsets = tc.bare_table([tc.random_bits((5, 3), rng)], lead=4, trail=0, rng=rng)
	(tmp_path / 'table.bin').write_bytes(table)
	head = f"unpack 1 {tmp_path / 'table.bin'} {tmp_path / 'out.bin'} {row_bytes} 5"
	assert driver(f'{head} 5 1 {offsets[0]} 0 0 0 3 48 -1')[0].startswith('refused tp_tpf_unpack: t_pitch')
	assert driver(f'{head} 2 1 {offsets[0]} 0 0 0 3 32 2 3 3')[0].startswith('refused tp_tpf_unpack: the kept rows')
	assert driver(f'{head} 5 1 {offsets[0] + 4} 0 0 0 3 32 -1')[0].startswith('refused tp_tpf_unpack: a column leaves the row')
	assert not (tmp_path / 'out.bin').exists()
	assert driver(f'{head} 2 1 {offsets[0]} 0 0 0 3 32 2 1 4') == ['ok writes 96 min 1 max 1']
