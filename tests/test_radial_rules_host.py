# -*- coding: utf-8 -*-
"""
CPU check of the radial background's device-free rules (photometry_amd/csrc/radial_rules.h, select_rules.h): the headers compiled for
the host with AddressSanitizer and UBSan into the driver tests/hostsim/radial_rules_host.cpp, which composes them serially the way
csrc/radial.hip composes them in parallel, held to numpy, scipy and the oracle: (a) the keys and the radix selection with the
next-order-statistic rule, the percentiles; (b) the pixel and sample rules; (c) a whole ring mode from a list of log samples against
``oracle.backgrounds.reduce_mode(binning='fixed')`` at the kernel's block and batch boundaries, at zero bandwidth and where there is
no mode; (d) the ring profile: moving median, knots, coefficients; (e) the spline's evaluation; (f) the host checks of the entries.
"""
import os
import subprocess
import warnings
import numpy as np
import pytest
import conftest
import radial_common as rc
from oracle import backgrounds as ob

CSRC = os.path.join(conftest.ROOT, 'photometry_amd', 'csrc')
SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'radial_rules_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'radial_rules_host')


@pytest.fixture(scope='module')
def driver():
	os.makedirs(OUT_DIR, exist_ok=True)
	subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall',
		'-I' + CSRC, '-o', OUT, SRC], check=True)

	def run(text):
		r = subprocess.run([OUT], input=text, capture_output=True, text=True, timeout=120)
		assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
		assert r.returncode == 0, (r.stdout[-2000:], r.stderr)
		assert r.stderr == '', r.stderr
		assert 'FAILED:' not in r.stdout, r.stdout[-2000:]
		return r.stdout.splitlines()
	return run


def _hex64(values):
	return ' '.join('%016x' % v for v in np.asarray(values, dtype='float64').ravel().view('uint64'))


def _hex32(values):
	return ['%08x' % v for v in np.asarray(values, dtype='float32').ravel().view('uint32')]


def _f64(words):
	return np.array([int(w, 16) for w in (words.split() if isinstance(words, str) else words)], dtype='uint64').view('float64')


@pytest.mark.parametrize('headers', (['radial_rules.h'], ['select_rules.h'], ['select_rules.h', 'radial_rules.h', 'halo_rules.h'], ['halo_rules.h', 'radial_rules.h']))
def test_headers_compile_alone(tmp_path, headers):
	src = tmp_path / 'only.cpp'
	src.write_text(''.join(f'#include "{h}"\n' for h in headers) + 'int main() { return (int)tp_select::okey(0.0); }\n')
	subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only', '-I' + CSRC, str(src)], check=True)


# ---- (a) keys, selection, percentiles -----------------------------------------------------------------------------------------------
def _series(kind, n, rng):
	if kind == 'random':
		return 2.0 + rng.normal(0, 2e-3, n)
	if kind == 'ties':                                                              # five values, two of them neighbours
		return rng.choice(np.array([3.5, -2.25, 1e-300, 7e8, 3.5000000000000004]), size=n)
	if kind == 'float32':                                                           # first-round samples: float32 logarithms, many equal
		return (2.0 + rng.normal(0, 3e-6, n)).astype('float32').astype('float64')
	return rng.normal(size=n) * 10.0**rng.integers(-3, 4, size=n)                   # mixed sign


def test_keys_keep_the_order_and_round_trip(driver):
	fi = np.finfo('float64')
	rng = np.random.default_rng(21)
	x = np.concatenate([[0.0, -0.0, np.inf, -np.inf, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max, -fi.max, 1.0, -1.0,
		np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)], rng.normal(size=5000) * 10.0**rng.integers(-30, 30, size=5000), _series('ties', 2000, rng)])
	out = driver(f'keys {len(x)} ' + _hex64(x))
	keys = np.array([int(line.split()[0], 16) for line in out], dtype='uint64')
	back = np.array([int(line.split()[1], 16) for line in out], dtype='uint64')
	assert np.array_equal(back, x.view('uint64'))                                  # the round trip is exact
	order = np.argsort(keys, kind='stable')
	assert np.array_equal(x[order], np.sort(x))                                    # numpy's order (-0 and +0 compare equal there)
	gt = np.diff(x[order]) > 0
	assert np.all(keys[order][1:][gt] > keys[order][:-1][gt]) and keys[1] < keys[0]
	assert np.array_equal(np.diff(keys[order]) == 0, np.diff(x[order].view('uint64').astype('int64')) == 0)


@pytest.mark.parametrize('kind', ['random', 'ties', 'float32', 'mixed'])
def test_serial_selection_of_quartile_and_median_ranks_equals_the_sorted_series(driver, kind):
	rng = np.random.default_rng(31)
	text, want = [], []
	for n in (1, 2, 3, 4, 255, 256, 257, 2047, 2048, 2049):
		x = _series(kind, n, rng)
		ks = sorted({0, int(0.25 * (n - 1)), (n - 1) // 2, n // 2, int(0.75 * (n - 1)), n - 1})
		text.append(f'select {n} {len(ks)} ' + _hex64(x) + ' ' + ' '.join(map(str, ks)))
		s = np.sort(x)
		want += [(s[k], s[min(k + 1, n - 1)]) for k in ks]                            # the order statistic and the next one
	got = [tuple(_f64(line)) for line in driver('\n'.join(text))]
	assert got == want


@pytest.mark.parametrize('kind', ['random', 'ties', 'float32'])
def test_percentiles_equal_scoreatpercentile(driver, kind):
	"""percentile_from_pair and the next-order-statistic rule against ``scipy.stats.scoreatpercentile`` at 25, 50 and 75 (what
	statsmodels' ``_select_sigma`` calls), odd and even ``n``, with duplicated neighbours ('ties', 'float32'); the median rule against
	``np.median``.  Exact: both sides interpolate ``(s0 w0 + s1 w1) / (w0 + w1)`` between the same two order statistics."""
	from scipy.stats import scoreatpercentile
	rng = np.random.default_rng(32)
	series = [_series(kind, n, rng) for n in (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 254, 255, 256, 257, 1001, 2048)]
	series += [np.array([1.0, 1.0, 2.0, 2.0]), np.array([1.0, 2.0, 2.0, 2.0, 3.0, 3.0]), np.array([5.0, 5.0, 5.0]), np.array([2.0, 1.0, 1.0, 3.0, 3.0, 1.0, 2.0])]
	out = driver('\n'.join(f'percentiles {len(x)} ' + _hex64(x) for x in series))
	for x, line in zip(series, out):
		want = [scoreatpercentile(x, p) for p in (25, 50, 75)] + [np.median(x)]
		assert list(_f64(line)) == want, (len(x), x[:8])


# ---- (b) pixels and samples ---------------------------------------------------------------------------------------------------------
def test_pixel_and_sample_rules(driver):
	cutoff = np.float32(8e4)
	x = np.array([0.0, -0.0, -1e-30, 1.0, 8e4, np.nextafter(cutoff, np.float32(np.inf)), np.nextafter(cutoff, np.float32(0)), np.nan, np.inf, -np.inf, 5.5], dtype='float32')
	cases = [(v, e) for v in x for e in (0, 1)]
	out = driver(f'pixel {_hex32(cutoff)[0]} {len(cases)} ' + ' '.join(f'{_hex32(v)[0]} {e}' for v, e in cases))
	with np.errstate(invalid='ignore'):
		assert [int(v) for v in out] == [int(bool(~ob.stamp_mask(np.array([v]), 8e4, np.array([bool(e)]))[0])) for v, e in cases]
	rng = np.random.default_rng(5)
	pix, sq = rng.uniform(0, 500, 200).astype('float32'), rng.uniform(0, 300, 200).astype('float32')
	out = driver(f'value {len(pix)} ' + ' '.join(f'{a} {b}' for a, b in zip(_hex32(pix), _hex32(sq))))
	got = np.array([_f64(line) for line in out])
	assert np.array_equal(got[:, 0], pix.astype('float64')) and np.array_equal(got[:, 1], pix.astype('float64') - sq.astype('float64'))
	# the log samples as fit_background_tess(device_arithmetic=True) forms them: first round float32(log10(float64(pix + zp in float32))),
	# later rounds log10(v + zp) in float64 (glibc's log10 against numpy's: 1 ulp)
	zp = 17.25
	v = (pix.astype('float64') - sq.astype('float64'))
	v = v - v.min()
	out = driver(f'logs {_hex64(zp)} {len(v)} ' + _hex64(v))
	got = np.array([_f64(line) for line in out])
	first = np.log10((v.astype('float32') + np.float32(zp)).astype('float64')).astype('float32')
	assert np.array_equal(got[:, 0], first.astype('float64'))
	np.testing.assert_allclose(got[:, 1], np.log10(v + zp), rtol=3e-16)
	out = driver(f'zeropoint 4 ' + _hex64([-3.5, 120.0, np.inf, 0.0]))
	np.testing.assert_array_equal(np.concatenate([_f64(line) for line in out]), [4.5, -119.0, np.nan, 1.0])


# ---- (c) the ring mode ----------------------------------------------------------------------------------------------------------------
RING_SIZES = (0, 1, 2, 3, 4, 255, 256, 257, 2047, 2048, 2049, 4097)


def _ring_modes(driver, series, zp=1.0):
	out = driver('\n'.join(f'mode {_hex64(rc.BW_CONSTANT)} {_hex64(zp)} {len(x)} ' + _hex64(x) for x in series))
	assert [int(line.split()[0]) for line in out] == [len(x) for x in series]
	return [(_f64(line.split()[1:2])[0], _f64(line.split()[2:3])[0]) for line in out]


def test_ring_mode_equals_the_oracle_at_the_block_and_batch_boundaries(driver):
	"""A whole ring mode composed serially from the rules against ``oracle.backgrounds.reduce_mode(x, binning='fixed')`` on
	``2.0 + normal(0, 2e-3, n)`` (seed 3) for ring sizes around the kernel's block (256) and batch (2048 = 8 x 256) boundaries: the same
	NaN pattern (n = 0 and 1) and the same grid point, no case left out -- radial_common says what "the same" is held to where the
	oracle's own argmax is a tie (n = 2) and asserts that it is none anywhere else."""
	series = [2.0 + np.random.default_rng(3).normal(0, 2e-3, n) for n in RING_SIZES]
	rules = []
	for x, (mode, bw) in zip(series, _ring_modes(driver, series)):
		with warnings.catch_warnings():
			warnings.simplefilter('ignore', RuntimeWarning)
			ref = ob.reduce_mode(x, binning='fixed')
			mine = rc.oracle_ring_mode(x)[0]
			assert ref == mine or (np.isnan(ref) and np.isnan(mine))                   # the restatement with its margin is the oracle's
			rules.append(rc.assert_same_mode(mode, x, label=len(x)))
		print(len(x), 'samples: mode', mode, 'oracle', ref, 'bandwidth', bw, rules[-1])
	assert rules == ['nan', 'nan', 'tie'] + ['argmax'] * 9
	# a NaN zero point (nothing unmasked in the frame): no mode whatever the samples
	assert np.isnan(_ring_modes(driver, series[5:6], zp=np.nan)[0][0])


def test_ring_mode_without_a_bandwidth_is_the_median(driver):
	"""All samples equal (odd and even n): ``bw == 0``, the mode is the median, exact.  And a ring whose inter-quartile range is 0
	but whose standard deviation is not: sigma = std, an ordinary mode."""
	v = float(np.float32(np.log10(151.0)))
	series = [np.full(n, v) for n in (2, 3, 256, 257, 2048, 2049)]
	for x, (mode, bw) in zip(series, _ring_modes(driver, series)):
		assert bw == 0.0 and mode == v and rc.assert_same_mode(mode, x) == 'median'
	rng = np.random.default_rng(8)
	x = np.full(301, 2.0)
	x[rng.choice(301, 60, replace=False)] = 2.0 + rng.normal(0, 2e-3, 60)               # 80 % equal: both quartiles are 2.0
	from scipy.stats import scoreatpercentile
	assert scoreatpercentile(x, 75) - scoreatpercentile(x, 25) == 0.0 and np.std(x, ddof=1) > 0
	(mode, bw), = _ring_modes(driver, [x])
	np.testing.assert_allclose(bw, rc.BW_CONSTANT * np.std(x, ddof=1) * 301**-0.2, rtol=1e-13)
	assert rc.assert_same_mode(mode, x, label='iqr 0') == 'argmax'


# ---- (d) the ring profile ---------------------------------------------------------------------------------------------------------------
def _nan_runs(n, rng, k):
	x = 2.0 + 0.01 * np.arange(n) + rng.normal(0, 2e-3, n)
	if k % 4 == 1:
		x[rng.random(n) < 0.3] = np.nan
	elif k % 4 == 2:
		a = int(rng.integers(0, n)); x[a:a + int(rng.integers(1, 6))] = np.nan         # a run
	elif k % 4 == 3:
		x[:int(rng.integers(0, n + 1))] = np.nan                                         # a leading run, up to everything
	return x


def test_moving_median_equals_the_oracle(driver):
	rng = np.random.default_rng(12)
	cases = [(w, _nan_runs(n, rng, n + w)) for w in (0, 3, 5, 8) for n in range(1, 65)]
	out = driver('\n'.join(f'median {w} {len(x)} ' + _hex64(x) for w, x in cases))
	from oracle import utilities as ou
	short = 0
	for (w, x), line in zip(cases, out):
		n = len(x)
		if w and n < w // 2 + 1:
			# the reference itself fails on a series this short (y[k] beyond the end, utilities.py:54-55); the rule stops at the series' end
			with pytest.raises(IndexError):
				ob.move_median_central(x, w)
			with warnings.catch_warnings():
				warnings.simplefilter('ignore', RuntimeWarning)
				want = np.roll(ou._move_median(x, w, min_count=1), -w // 2 + 1)
				for k in range(n):
					want[k] = ou._nanmedian(x[:k + 2])
					want[n - 1 - k] = ou._nanmedian(x[-(k + 2):])
			short += 1
		else:
			want = ob.move_median_central(x, w) if w else x
		np.testing.assert_array_equal(_f64(line), want, err_msg=f'width {w}, {n} points')
	assert short == 1 + 2 + 4


def _profile_patterns():
	"""The nine ``s2`` patterns of test_mesh_finish_and_ring_profiles_on_device, 64 rings, exactly 4 (and 3) usable rings."""
	rng = np.random.default_rng(21)
	nr = 39
	bc = 2400.0 + 15.0 * np.arange(nr) + 7.5
	s2 = 2.0 + 0.004 * np.arange(nr)[None, :] + rng.normal(0, 2e-3, (9, nr))
	s2[1, 0] = np.nan; s2[1, 17:20] = np.nan; s2[1, -1] = np.nan
	s2[2, :] = np.nan; s2[2, 5] = 2.0; s2[2, 6] = 2.1
	s2[3, :] = np.nan; s2[3, 3:8] = [2.0, 2.1, 2.05, 2.2, 2.15]
	s2[4, ::2] = np.nan
	s2[5, :] = np.nan; s2[5, [4, 20, 30]] = 2.0
	cases = [(bc, row) for row in s2]
	bc64 = 2400.0 + 15.0 * np.arange(64) + 7.5
	full = 2.0 + 0.3 * np.sin(bc64 / 100.0) + rng.normal(0, 2e-3, 64)
	gaps = full.copy(); gaps[[0, 1, 30, 31, 32, 63]] = np.nan
	four = np.full(64, np.nan); four[[2, 9, 40, 63]] = [2.0, 2.2, 2.1, 2.4]
	three = four.copy(); three[9] = np.nan
	return cases + [(bc64, full), (bc64, gaps), (bc64, four), (bc64, three)]


def test_ring_profile_equals_fitpack(driver):
	"""Knots exact, coefficients at the tolerance of the device test, ``n_knots == 0`` exactly where fewer than 4 rings are usable."""
	from scipy.interpolate import InterpolatedUnivariateSpline
	cases = [(smooth, bc, s2) for smooth in (3, 0, 5) for bc, s2 in _profile_patterns()]
	text = [f'profile {w} {len(bc) + 4} {len(bc)} ' + ' '.join(f'{_hex64(b)} {_hex64(s)}' for b, s in zip(bc, s2)) for w, bc, s2 in cases]
	out = driver('\n'.join(text))
	none = 0
	for k, (w, bc, s2) in enumerate(cases):
		n, kn, co = int(out[3 * k]), _f64(out[3 * k + 1]), _f64(out[3 * k + 2])
		prof = ob.move_median_central(s2, w) if w else s2
		good = ~np.isnan(prof)
		if good.sum() < 4:
			assert n == 0 and len(kn) == 0
			none += 1
			continue
		t, c, _ = InterpolatedUnivariateSpline(bc[good], prof[good], k=3, ext=3)._eval_args
		m = int(good.sum())
		assert n == len(t) == m + 4 and (w == 0 and m == 4 or m > 4 or w > 0)
		np.testing.assert_array_equal(kn, t)
		np.testing.assert_allclose(co, c[:m], rtol=1e-11, atol=1e-12)
	assert none >= 3
	# exactly 4 usable rings give a spline (without smoothing: the medians would fill their neighbours), 3 do not
	bc, four = _profile_patterns()[-2]
	assert int(driver(f'profile 0 68 64 ' + ' '.join(f'{_hex64(b)} {_hex64(s)}' for b, s in zip(bc, four)))[0]) == 8
	# more knots than the caller's arrays hold: no radial component
	assert int(driver(f'profile 0 7 64 ' + ' '.join(f'{_hex64(b)} {_hex64(s)}' for b, s in zip(bc, four)))[0]) == 0


# ---- (e) the spline's evaluation ----------------------------------------------------------------------------------------------------------
def test_spline_evaluation_equals_scipy(driver):
	"""``10**spline(r) - zeropoint`` on radii inside, on and beyond the end knots (ext = 3) against scipy's spline: after the float32
	store at the tolerance of test_radial_pieces; in float64 the deviation measured against scipy is 2.2e-13 relative to
	``10**spline`` (the reciprocals, ``exp10`` against ``10**``), held to 2e-12."""
	from scipy.interpolate import InterpolatedUnivariateSpline
	xcen, ycen, off, zp = 2158.222313, 2099.523364, 44.0, 7.5
	x = 2400.0 + 15.0 * np.arange(39) + 7.5
	y = 2.0 + 0.3 * np.sin(x / 100.0)
	for keep in (np.r_[0:3, 5:17, 18:39], np.array([2, 9, 20, 38])):                    # 36 rings; exactly 4
		spl = InterpolatedUnivariateSpline(x[keep], y[keep], k=3, ext=3)
		t, c, _ = spl._eval_args
		# pixels: along the diagonal away from the centre (inside the first knot .. beyond the last), and on the end knots' row
		cols = np.concatenate([np.arange(0, 2048, 37), [0, 2047]])
		rows = np.concatenate([np.arange(0, 2048, 37)[::-1] // 2, [0, 0]])
		text = f'evaluate {len(t)} {_hex64(t)} {_hex64(c)} {_hex64(zp)} {_hex64(off)} {_hex64(xcen)} {_hex64(ycen)} {len(cols)} ' + ' '.join(f'{r} {q}' for r, q in zip(rows, cols))
		out = driver(text)
		r = np.sqrt((cols + off - xcen)**2 + (rows - ycen)**2)
		assert r.min() < t[0] and r.max() > t[-1]
		ref = 10**spl(r) - zp
		got32 = np.array([int(line.split()[0], 16) for line in out], dtype='uint32').view('float32')
		got64 = np.array([_f64(line.split()[1:2])[0] for line in out])
		np.testing.assert_allclose(got32, ref, rtol=2e-7, atol=1e-5)
		dev = np.max(np.abs(got64 - ref) / (ref + zp))
		print(len(keep), 'rings: float64 deviation from scipy relative to 10**spline', dev)
		assert dev < 2e-12
	# on the end knots exactly, and no radial component below 8 knots
	text = f'evaluate {len(t)} {_hex64(t)} {_hex64(c)} {_hex64(zp)} {_hex64(0.0)} {_hex64(0.0)} {_hex64(0.0)} 2 0 {int(t[0] + 0.5)} 0 {int(t[-1] + 0.5)}'
	got = np.array([_f64(line.split()[1:2])[0] for line in driver(text)])
	np.testing.assert_allclose(got, 10**spl(np.array([int(t[0] + 0.5), int(t[-1] + 0.5)], dtype='float64')) - zp, rtol=2e-12)
	text = f'evaluate 7 {_hex64(t[:7])} {_hex64(c[:7])} {_hex64(zp)} {_hex64(off)} {_hex64(xcen)} {_hex64(ycen)} 1 5 5'
	assert _f64(driver(text)[0].split()[1:2])[0] == 0.0


# ---- (f) host checks ------------------------------------------------------------------------------------------------------------------
def test_entry_checks_and_band_division(driver):
	ask = lambda text: [int(v) for v in driver(text)[0].split()]
	for args, ok in (((1, 100, 100), 1), ((0, 100, 100), 1), ((65535, 100, 101), 1), ((65536, 100, 100), 0), ((-1, 100, 100), 0), ((1, 0, 0), 0),
			((1, 100, 99), 0), ((1, 2**31 - 1, 2**31 - 1), 1), ((1, 2**31, 2**31), 0)):
		assert ask('imageok ' + ' '.join(map(str, args))) == [ok], args
	# have, mesh_rows, mesh_cols, box, frame_cols, n_pixels: the mesh must reach the last row and column
	for args, ok in (((1, 5, 7, 64, 421, 300 * 421), 1), ((0, 5, 7, 64, 421, 300 * 421), 0), ((1, 4, 7, 64, 421, 300 * 421), 0), ((1, 5, 6, 64, 421, 300 * 421), 0),
			((1, 5, 7, 64, 421, 300 * 421 + 1), 0), ((1, 5, 7, 0, 421, 300 * 421), 0), ((1, 0, 7, 64, 421, 300 * 421), 0), ((1, 5, 7, 64, 0, 300 * 421), 0),
			((1, 32, 32, 64, 2048, 2048 * 2048), 1)):
		assert ask('zoomok ' + ' '.join(map(str, args))) == [ok], args
	for args, ok in (((0, 5, 100), 1), ((1, 0, 100), 1), ((1, 100, 100), 1), ((1, 99, 100), 0), ((1, 1000, 100), 1)):
		assert ask('sideok ' + ' '.join(map(str, args))) == [ok], args
	# n_rows, n_partial, col_blocks -> fits, bands, rows per band: n_partial smaller than, equal to and larger than the column blocks
	assert ask('bands 2048 7 8') == [0, 0, 0]                                           # no row of workgroups fits: the flat walk
	assert ask('bands 2048 8 8') == [1, 1, 2048]
	assert ask('bands 2048 256 8') == [1, 32, 64]
	assert ask('bands 300 256 2') == [1, 100, 3]                                       # 128 bands asked: 3 rows each, 100 bands cover 300 rows
	assert ask('bands 5 256 1') == [1, 5, 1]                                            # more bands than rows
	assert ask('bands 1 65535 1') == [1, 1, 1]
	for n_rows, n_partial, col_blocks in ((2048, 256, 8), (300, 256, 2), (301, 17, 3), (5, 256, 1), (77, 9, 2)):
		fits, bands, per = ask(f'bands {n_rows} {n_partial} {col_blocks}')
		assert fits == 1 and bands * col_blocks <= n_partial and bands * per >= n_rows and (bands - 1) * per < n_rows
