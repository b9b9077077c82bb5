# -*- coding: utf-8 -*-
"""
The device-free side of LinPSF photometry on batches of target pixel files: ``tpf.jitter_lookup`` against the plugin's ``argmin`` taken
cadence by cadence; the device-free rules of ``tp_star_positions_targets`` (photometry_amd/csrc/starpos_rules.h) compiled for the host
with AddressSanitizer and UBSan into tests/hostsim/starpos_host.cpp, which composes them serially -- every block, every thread, every
star a block walks -- over arrays that hold exactly the values a call may touch, held bit for bit to the numpy restatement of
tests/tpf_linpsf_common.py; and the method check of ``tessphot_tpfs``.
"""
import os
import subprocess
import numpy as np
import pytest
import conftest
import tpf_linpsf_common as lc
from photometry_amd import tpf, tessphot_tpfs

SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'starpos_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'starpos_host')


# ---- the lookup ----------------------------------------------------------------------------------------------------------------------
def _hold_lookup(time, timecorr):
	want = lc.argmin_lookup(time, timecorr)
	got = tpf.jitter_lookup(time, timecorr)
	if np.array_equal(want, np.arange(len(want))):
		assert got is None
	else:
		assert got is not None and got.dtype == np.int32 and got.shape == want.shape
		np.testing.assert_array_equal(got, want)
	return got


@pytest.mark.parametrize('name', sorted(lc.hand_cases()))
def test_jitter_lookup_hand_cases(name):
	time, timecorr = lc.hand_cases()[name]
	got = _hold_lookup(time, timecorr)
	T = len(time)
	if name in ('increasing', 'decreasing_pair', 'single', 'inf'):
		# distinct finite values: every cadence is its own nearest; one infinite tref is the only NaN of its own differences
		assert got is None
	elif name == 'nan_first':
		assert got.tolist() == [0] * T                                   # numpy's argmin returns the first NaN
	elif name == 'nan_middle':
		# (at the NaN's own cadence every difference is NaN: the first of them is cadence 0)
		assert got.tolist() == [5] * 5 + [0] + [5] * (T - 6)
	elif name == 'two_nans':
		assert got.tolist() == [4] * 4 + [0] + [4] * 4 + [0] + [4] * (T - 10)
	elif name == 'two_equal':
		assert got.tolist() == [0, 1, 2, 3, 4, 5, 6, 3, 8, 9, 10, 11]     # the first of the equal ones


def test_jitter_lookup_random_vectors():
	seen = 0
	for time, timecorr in lc.random_cases():
		assert len(time) <= 40
		seen += _hold_lookup(time, timecorr) is not None
	assert seen >= 10


def test_jitter_lookup_common_case_is_linear():
	"""19 000 strictly increasing cadences: identity without the T x T differences (a second, not minutes)."""
	T = 19000
	time = 1683.35 + np.arange(T) * (120.0 / 86400.0)
	assert tpf.jitter_lookup(time, np.full(T, 3e-3, dtype='float32')) is None
	time[12000] = time[100]
	got = tpf.jitter_lookup(time, np.zeros(T, dtype='float32'))
	assert got[12000] == 100 and np.array_equal(np.delete(got, 12000), np.delete(np.arange(T), 12000))


# ---- the position rule ---------------------------------------------------------------------------------------------------------------
def test_numpy_restatement_is_the_plugins_expression():
	"""``positions_numpy`` against ``BasePhotometry.catalog_attime`` + the plugin's loop written out on arrays."""
	base, star_target, shift, lookup = lc.kernel_case(T=40, seed=1)
	got = lc.positions_numpy(base, star_target, shift, 40, lookup=lookup, pos_pitch=43)
	for s, t in enumerate(star_target):
		rows = np.arange(40) if lookup[t] is None else lookup[t]
		col = np.empty(40)
		for k in range(40):
			cat = np.array([base[s]], dtype='float32')
			cat = cat + np.float32(shift[t, rows[k]])                      # BasePhotometry.catalog_attime
			assert cat.dtype == np.float32
			col[k] = cat[0]                                                  # do_photometry: pos_row[:, k] = ...
		np.testing.assert_array_equal(lc.bits(got[s, :40]), lc.bits(col))
	assert np.all(lc.bits(got[:, 40:]) == lc.SENTINEL_BITS)
	assert np.isnan(got[star_target == 1][:, [0, 20, 39]]).all() and np.isnan(got[:, :40]).sum() == 3 * 3
	# the float32 sum rounds: it is not the float64 sum
	assert np.any(got[:, :40] != base[:, None].astype('float64') + shift[star_target][:, :40])


# ---- the rules under the sanitizers --------------------------------------------------------------------------------------------------
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


def _positions(driver, base, star_target, shift, n_cad, lookup=None, pos_pitch=None, lookup_pitch=None, n_stars=None, n_targets=None, shift_pitch=None, null=0):
	"""One ``positions`` command: the answer line and the float64 ``(n_stars, pos_pitch)`` array (None when refused).  ``lookup``: the whole
	int32 ``(n_targets, lookup_pitch)`` array or None."""
	base = np.asarray(base, dtype='float32')
	shift = np.asarray(shift, dtype='float64')
	n_stars = len(base) if n_stars is None else n_stars
	n_targets = shift.shape[0] if n_targets is None else n_targets
	shift_pitch = shift.shape[1] if shift_pitch is None else shift_pitch
	pos_pitch = n_cad if pos_pitch is None else pos_pitch
	lookup_pitch = (0 if lookup is None else lookup.shape[1]) if lookup_pitch is None else lookup_pitch
	words = ['positions 1', str(n_stars), str(n_cad), str(n_targets), str(shift_pitch), '0' if lookup is None else '1', str(lookup_pitch), str(pos_pitch), str(null)]
	words += ['%08x' % v for v in base.view('uint32')[:max(n_stars, 0)]]
	words += [str(int(v)) for v in np.asarray(star_target)[:max(n_stars, 0)]]
	words += ['%016x' % v for v in shift.view('uint64').ravel()[:max(n_targets, 0) * max(shift_pitch, 0)]]
	if lookup is not None:
		words += [str(int(v)) for v in np.asarray(lookup).ravel()[:max(n_targets, 0) * max(lookup_pitch, 0)]]
	lines = driver(' '.join(words) + '\n')
	if lines[0].startswith('refused'):
		assert len(lines) == 1
		return lines[0], None
	rows = [[int(w, 16) for w in line.split()] for line in lines[1:]]
	return lines[0], np.array(rows, dtype='uint64').reshape(len(rows), pos_pitch if rows else 0).view('float64')


def test_grid_owns_every_pair_once(driver):
	assert driver('grid 1') == ['ok']


@pytest.mark.parametrize('name', sorted(lc.hand_cases()))
def test_rules_compose_to_the_restatement_on_the_hand_cases(driver, name):
	"""Two targets with the case's time axis, three stars: target 0 through the case's lookup (NULL when it is the identity), target 1
	with NaN shifts; whole-array lookup with an identity row for target 1."""
	time, timecorr = lc.hand_cases()[name]
	T = len(time)
	rng = np.random.default_rng(T + len(name))
	look = tpf.jitter_lookup(time, timecorr)
	base = (5.5 + rng.normal(size=3)).astype('float32')
	star_target = np.array([1, 0, 1], dtype='int32')
	shift = rng.uniform(1e-3, 0.3, size=(2, T)) * rng.choice([-1.0, 1.0], size=(2, T))
	shift[1, ::5] = np.nan
	whole = None if look is None else np.stack([look, np.arange(T, dtype='int32')]).astype('int32')
	line, got = _positions(driver, base, star_target, shift, T, lookup=whole, pos_pitch=T + 3)
	assert line == 'ok writes %d max 1' % (3 * T), line
	want = lc.positions_numpy(base, star_target, shift, T, lookup=[look, None], pos_pitch=T + 3)
	np.testing.assert_array_equal(lc.bits(got), lc.bits(want))
	# ... and held to the plugin's own index, not to jitter_lookup's
	np.testing.assert_array_equal(lc.bits(got), lc.bits(lc.positions_numpy(base, star_target, shift, T, lookup=[lc.argmin_lookup(time, timecorr), None], pos_pitch=T + 3)))


@pytest.mark.parametrize('T,pitch', [(300, 320), (1, 1), (256, 256), (257, 300)])
def test_rules_compose_to_the_restatement_on_the_kernel_shapes(driver, T, pitch):
	base, star_target, shift, lookup = lc.kernel_case(T=T, pos_pitch=pitch)
	line, got = _positions(driver, base, star_target, shift, T, pos_pitch=pitch)
	assert line == 'ok writes %d max 1' % (len(base) * T)
	np.testing.assert_array_equal(lc.bits(got), lc.bits(lc.positions_numpy(base, star_target, shift, T, pos_pitch=pitch)))
	whole = np.stack([np.arange(T, dtype='int32') if v is None else v for v in lookup]).astype('int32')
	line, got = _positions(driver, base, star_target, shift, T, lookup=whole, pos_pitch=pitch)
	assert line.startswith('ok')
	np.testing.assert_array_equal(lc.bits(got), lc.bits(lc.positions_numpy(base, star_target, shift, T, lookup=lookup, pos_pitch=pitch)))


def test_values_that_point_outside_their_array_are_not_followed(driver):
	"""A star of no target and a lookup row outside the series: NaN, no read (the arrays hold exactly what may be read)."""
	base = np.array([1.5, 2.5, 3.5], dtype='float32')
	shift = np.array([[0.25, 0.5, 0.75, 1.0]])
	look = np.array([[0, 4, -1, 3]], dtype='int32')
	line, got = _positions(driver, base, [0, 1, -1], shift, 4, lookup=look)
	assert line == 'ok writes 12 max 1'
	assert got[0].tolist()[0] == 1.75 and got[0].tolist()[3] == 2.5 and np.isnan(got[0, 1:3]).all() and np.isnan(got[1:]).all()


REFUSALS = {
	'negative stars': dict(n_stars=-1), 'negative cadences': dict(n_cad=-1), 'pos_pitch below n_cad': dict(pos_pitch=3), 'no targets': dict(n_targets=0),
	'shift_pitch below n_cad': dict(shift_pitch=3), 'lookup_pitch below n_cad': dict(with_lookup=True, lookup_pitch=3),
	'shift_pitch 0 with a lookup': dict(with_lookup=True, shift_pitch=0), 'null base': dict(null=1), 'null star_target': dict(null=2), 'null shift': dict(null=3),
	'null output': dict(null=4)}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_refusals(driver, name):
	kw = dict(REFUSALS[name])
	base, shift = np.array([1.5, 2.5], dtype='float32'), np.arange(8, dtype='float64').reshape(2, 4)
	lookup = np.zeros((2, 4), dtype='int32') if kw.pop('with_lookup', False) else None
	n_cad = kw.pop('n_cad', 4)
	line, got = _positions(driver, base, [0, 1], shift, n_cad, lookup=lookup, **kw)
	assert line.startswith('refused tp_star_positions_targets: ') and got is None, (name, line)


def test_empty_calls_are_taken_without_pointers(driver):
	base, shift = np.array([1.5, 2.5], dtype='float32'), np.arange(8, dtype='float64').reshape(2, 4)
	line, got = _positions(driver, base, [0, 1], shift, 4, n_stars=0, null=1)
	assert line == 'ok writes 0 max 0'
	line, got = _positions(driver, base, [0, 1], shift, 0, pos_pitch=2, null=4)
	assert line == 'ok writes 0 max 0' and np.all(lc.bits(got) == lc.SENTINEL_BITS)


# ---- the entry -----------------------------------------------------------------------------------------------------------------------
def test_psf_is_still_an_invalid_method(tmp_path):
	missing = str(tmp_path / 'no-such-file_tp.fits')
	with pytest.raises(ValueError, match=r"Invalid method: 'psf'"):
		list(tessphot_tpfs(None, [missing], {}, method='psf'))
	with pytest.raises(ValueError, match=r"Invalid method: 'linpsf '"):
		list(tessphot_tpfs(None, [missing], {}, method='linpsf '))
