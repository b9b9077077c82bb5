# -*- coding: utf-8 -*-
"""
CPU check of the per-stamp flag series' device-free rules (photometry_amd/csrc/stampflags_rules.h): the header compiled for the host
with AddressSanitizer and UBSan into the driver tests/hostsim/stampflags_rules_host.cpp, which composes the rules serially -- every
block of the grid, every wavefront, every lane -- into a complete series, held to ``np.any(flags[:, r1:r2, c1:c2] & bit, axis=(1, 2))``
on the shapes of tests/stampflags_common.py, refusals included.  The flags file holds exactly the bytes a call may read, so a read
past the last frame is a sanitizer report.
"""
import os
import subprocess
import numpy as np
import pytest
import conftest
import stampflags_common as sc

SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'stampflags_rules_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'stampflags_rules_host')


@pytest.fixture(scope='module')
def driver():
	os.makedirs(OUT_DIR, exist_ok=True)
	subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall',
		'-I' + os.path.join(conftest.ROOT, 'photometry_amd', 'csrc'), '-o', OUT, SRC], check=True)

	def run(text):
		r = subprocess.run([OUT], input=text, capture_output=True, text=True, timeout=120)
		assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
		assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
		assert r.stderr == '', r.stderr
		return r.stdout.splitlines()
	return run


def _series(driver, tmp_path, raw, n_frames, R, C, stride, stamps, out_pitch, row0=sc.ROW0, col0=sc.COL0, flag_mask=sc.BIT, out_value=sc.OUT_VALUE,
		n_targets=None, null=0):
	"""One ``series`` command: the answer line and the output ``(n_targets, out_pitch)`` int32 (None when refused)."""
	fin, fout = tmp_path / 'flags.bin', tmp_path / 'out.bin'
	np.asarray(raw, dtype='uint8').tofile(fin)
	if fout.exists():
		fout.unlink()
	n = len(stamps) if n_targets is None else n_targets
	text = 'series 1 %s %s %d %d %d %d %d %d %d %d %d %d %d\n%s' % (fin, fout, n_frames, R, C, stride, row0, col0, n, flag_mask, out_value, out_pitch, null,
		'\n'.join(' '.join(str(int(v)) for v in s) for s in stamps[:max(n, 0)]))
	lines = driver(text)
	assert len(lines) == 1
	if lines[0].startswith('refused'):
		assert not fout.exists()
		return lines[0], None
	return lines[0], np.fromfile(fout, dtype='int32').reshape(n, out_pitch)


def test_lane_map_and_grid_cover_everything_once(driver):
	assert driver('maps 1') == ['ok']


@pytest.mark.parametrize('kind', ['clear', 'other_bits', 'sparse', 'everywhere'])
@pytest.mark.parametrize('pad', [0, 13])
@pytest.mark.parametrize('R,C', sc.REGIONS)
@pytest.mark.parametrize('T', [1, 2, 65])
def test_series_equals_numpy(driver, tmp_path, T, R, C, pad, kind):
	flags = sc.make_flags(kind, T, R, C, seed=T + R)
	if kind == 'sparse':
		flags[T // 2, R // 2, C // 2] |= sc.BIT          # (at density 1e-3 the small region may hold none)
	raw, stride = sc.with_stride(flags, pad)
	stamps = sc.region_stamps(R, C)
	pitch = T + 3
	line, out = _series(driver, tmp_path, raw, T, R, C, stride, sc.to_ccd(stamps), pitch)
	assert line == 'ok writes %d max 1' % (len(stamps) * T), line
	want = sc.expected(flags, [tuple(s) for s in stamps])
	np.testing.assert_array_equal(out[:, :T], want)
	assert np.all(out[:, T:] == sc.SENTINEL)
	if kind in ('clear', 'other_bits'):
		assert not want.any()
	else:
		assert want.any()


def test_flagged_pixels_just_outside_a_stamp(driver, tmp_path):
	flags, stamps = sc.neighbours_case()
	raw, stride = sc.with_stride(flags, 13)
	line, out = _series(driver, tmp_path, raw, 10, 40, 130, stride, sc.to_ccd(stamps), 10)
	assert line.startswith('ok')
	np.testing.assert_array_equal(out, sc.expected(flags, [tuple(s) for s in stamps]))
	assert out[0].tolist() == [0] * 9 + [sc.OUT_VALUE] and out[1].tolist() == [sc.OUT_VALUE] * 10


def test_one_flagged_frame_and_the_first_and_last_pixel_of_a_frame(driver, tmp_path):
	flags, stamps = sc.single_frames_case()
	raw, stride = sc.with_stride(flags, 0)
	line, out = _series(driver, tmp_path, raw, 65, 40, 130, stride, sc.to_ccd(stamps), 65)
	assert line.startswith('ok')
	np.testing.assert_array_equal(out, sc.expected(flags, [tuple(s) for s in stamps]))
	assert [np.flatnonzero(o).tolist() for o in out] == [[16], [31], [64], [16, 31, 64], [], [], [16]]


def test_a_mask_of_several_bits_and_another_output_value(driver, tmp_path):
	flags = sc.make_flags('sparse', 5, 5, 7, seed=3)
	raw, stride = sc.with_stride(flags, 0)
	stamps = sc.region_stamps(5, 7)
	line, out = _series(driver, tmp_path, raw, 5, 5, 7, stride, sc.to_ccd(stamps), 5, flag_mask=2 | 4 | 0x100, out_value=-7)
	assert line.startswith('ok')
	np.testing.assert_array_equal(out, sc.expected(flags, [tuple(s) for s in stamps], bit=6, out_value=-7))


@pytest.mark.parametrize('name', sorted(sc.REFUSALS))
def test_refusals(driver, tmp_path, name):
	kw = sc.refusal_base()
	kw.update(sc.REFUSALS[name])
	flags = kw.pop('flags')
	line, out = _series(driver, tmp_path, flags.ravel(), kw['n_frames'], kw['frame_rows'], kw['frame_cols'], kw['frame_stride'], np.asarray(kw['stamps'], dtype='int64'),
		kw['out_pitch'], flag_mask=kw['flag_mask'], n_targets=kw.get('n_targets'), null=kw['null'])
	assert line.startswith('refused tp_stamp_flag_series: ') and out is None, (name, line)


def test_the_good_call_of_the_refusals_is_taken(driver, tmp_path):
	kw = sc.refusal_base()
	line, out = _series(driver, tmp_path, kw['flags'].ravel(), 2, 5, 7, 35, np.asarray(kw['stamps'], dtype='int64'), 3)
	assert line == 'ok writes 4 max 1'
	assert out.tolist() == [[sc.OUT_VALUE, sc.OUT_VALUE, sc.SENTINEL]] * 2
