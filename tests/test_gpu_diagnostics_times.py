# -*- coding: utf-8 -*-
"""
``tp_lightcurve_diagnostics_times``: the light-curve diagnostics with one time vector per target (light curves of target pixel
files share their length, not their barycentric time stamps).  Row ``i`` of one strided launch is held bit for bit to the
shared-time entry run on target ``i`` alone with its own vector, and to ``oracle.diagnostics.diagnostics`` with the tolerances
of tests/test_gpu_diagnostics.py (``diagnostics_common.check``); stride 0 through the new entry is the old entry; both
residencies of the series (LDS, and the HBM scratch of long light curves); the two refused strides.

The time vectors are built so that they bin differently: 1300 s cadences (2.8 samples per one-hour bin), and a gap that puts the
next sample half a day after the last one, which is no whole number of bins later, so that every bin behind the gap regroups.
A guard on the oracle shows that the light curves tell the vectors apart.  A single NaN among the time stamps is skipped by the
reference (``nanmin`` / ``nanmax``, utilities.py:248-254) and sets no flag; an infinite one is the ``BAD_TIME`` flag, which the
long-light-curve case carries on one target only.
"""
import ctypes
import numpy as np
import pytest
import diagnostics_common as dc

gpu = pytest.mark.gpu    # (per test: the guard runs on the oracle alone)

CADENCE = 1300.0 / 86400.0


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def four_times(T, rng):
	"""Regular, with a half-day gap in the middle, shifted by 0.3 d, with one NaN."""
	base = 1400.0 + np.arange(T) * CADENCE + rng.normal(0, 1e-6, T)
	gap = base.copy()
	gap[T // 2:] += 0.5 - CADENCE
	shifted = base + 0.3
	nan = base.copy()
	nan[T // 3] = np.nan
	return np.stack((base, gap, shifted, nan))


def small_case():
	rng = np.random.default_rng(2024)
	Nt, T = 4, 70
	times = four_times(T, rng)
	flux, ferr, cen = dc.ordinary(rng, Nt, T)
	quality = np.zeros((Nt, T), dtype='int32')
	quality[rng.random((Nt, T)) < 0.06] = 32
	quality[rng.random((Nt, T)) < 0.04] = 16 # not in the default bitmask
	return times, quality, flux, ferr, cen


def oracle_row(time, quality, flux, ferr, cen, **extra):
	from oracle import diagnostics as odiag
	return odiag.diagnostics(time, quality, flux, ferr, cen, **extra)


def same_bits(a, b):
	return np.array_equal(np.ascontiguousarray(a).view('uint64'), np.ascontiguousarray(b).view('uint64'))


def test_guard_the_light_curves_tell_the_time_vectors_apart():
	"""On the oracle, on the CPU: ``rms_hour`` of a target changes under its neighbour's time vector -- for the regular and the
	gapped vector with a number on both sides."""
	times, quality, flux, ferr, cen = small_case()
	changed = 0
	for i in range(4):
		j = (i + 1) % 4
		own = oracle_row(times[i], quality[i], flux[i], ferr[i], cen[i])['rms_hour']
		other = oracle_row(times[j], quality[i], flux[i], ferr[i], cen[i])['rms_hour']
		changed += int(np.isfinite(own) and np.isfinite(other) and own != other)
	assert changed >= 2, changed
	a = oracle_row(times[0], quality[0], flux[0], ferr[0], cen[0])['rms_hour']
	b = oracle_row(times[1], quality[0], flux[0], ferr[0], cen[0])['rms_hour']
	assert np.isfinite(a) and np.isfinite(b) and abs(a - b) > 1e-3 * a, (a, b)


@gpu
def test_four_targets_four_time_vectors(ctx):
	times, quality, flux, ferr, cen = small_case()
	got = dc.run(ctx, times, quality, flux, ferr, cen)
	assert got.shape == (4, 10)
	for i in range(4):
		alone = dc.run(ctx, times[i], quality[i], flux[i:i + 1], ferr[i:i + 1], cen[i:i + 1])
		assert same_bits(got[i], alone[0]), (i, got[i], alone[0])
		dc.check(got[i], oracle_row(times[i], quality[i], flux[i], ferr[i], cen[i]), tag=f'target{i}')
	# and not what one shared vector gives
	shared = dc.run(ctx, times[0], quality, flux, ferr, cen)
	assert same_bits(got[0], shared[0]) and not same_bits(got[1], shared[1])


def _call(ctx, entry, Nt, T, lc, d_time, stride, d_q, out, d_status=None):
	args = [ctx.handle, Nt, T, lc.ptrs[0], lc.ptrs[1], lc.ptrs[3], lc.ptrs[4], lc.n_cad, d_time.ptr]
	if entry == 'tp_lightcurve_diagnostics_times':
		args.append(stride)
	args += [d_q.ptr, T, dc.DEFAULT_BITMASK, None if d_status is None else d_status.ptr, None, None, 0, 0, ctypes.c_double(dc.HOUR), out.ptr]
	return getattr(ctx.lib, entry)(*args)


def _light_curves(ctx, flux, ferr, cen):
	from photometry_amd import engine
	Nt, T = flux.shape
	lc = engine.LightCurves(ctx, Nt, T)
	block = np.zeros((5, Nt, T))
	block[0], block[1], block[3], block[4] = flux, ferr, cen[..., 0], cen[..., 1]
	ctx._check(ctx.lib.tp_memcpy_h2d(ctx.handle, lc.block.ptr, np.ascontiguousarray(block).ctypes.data, block.nbytes))
	return lc


@gpu
def test_stride_zero_is_the_shared_time_entry(ctx):
	times, quality, flux, ferr, cen = small_case()
	Nt, T = flux.shape
	lc = _light_curves(ctx, flux, ferr, cen)
	d_time, d_q = ctx.array(times[1]), ctx.array(quality)
	old, new = ctx.empty((Nt, 10), 'float64'), ctx.empty((Nt, 10), 'float64')
	assert _call(ctx, 'tp_lightcurve_diagnostics', Nt, T, lc, d_time, None, d_q, old) == 0
	assert _call(ctx, 'tp_lightcurve_diagnostics_times', Nt, T, lc, d_time, 0, d_q, new) == 0
	ctx.sync()
	a, b = old.to_host(), new.to_host()
	assert same_bits(a, b) and np.isfinite(a[:, 2]).all()
	# a pitched block of time vectors: stride above n_cad, the padding never read (NaN there would flag nothing; 1e30 would move tmax)
	pad = 5
	wide = np.full((Nt, T + pad), 1e30)
	wide[:, :T] = times
	d_wide = ctx.array(wide)
	pitched = ctx.empty((Nt, 10), 'float64')
	assert _call(ctx, 'tp_lightcurve_diagnostics_times', Nt, T, lc, d_wide, T + pad, d_q, pitched) == 0
	ctx.sync()
	assert same_bits(pitched.to_host(), dc.run(ctx, times, quality, flux, ferr, cen))


@gpu
def test_long_light_curves_in_hbm_scratch(ctx):
	"""Three targets at the smallest ``n_cad`` whose series arrays leave the LDS (``shmem > 160 * 1024`` in the host entry, restated in
	``diagnostics_common.lds_boundary``), three distinct time vectors, one of them with an infinite stamp: ``BAD_TIME`` on that row only."""
	T = dc.lds_boundary() + 1
	assert 6600 < T < 6700
	time, quality, flux, ferr, cen, kwargs, S, mask = dc.boundary_case(T)
	other = time.copy()
	other[T // 3:] += 0.77
	bad = time + 0.3
	bad[100] = np.inf
	times = np.stack((time, other, bad))
	assert not np.array_equal(times[0], times[1]) and not np.array_equal(times[0], times[2])
	quality = np.stack((quality, np.roll(quality, 5), np.roll(quality, 11)))
	status = np.ones(3, dtype='int32')
	got = dc.run(ctx, times, quality, flux, ferr, cen, status=status, sumimage=S, mask=mask)
	from photometry_amd.engine import DIAGNOSTICS_COLUMNS as COLS
	flags = got[:, COLS.index('flags')].astype(int)
	assert list(flags & 4) == [0, 0, 4], flags
	for i in range(3):
		alone = dc.run(ctx, times[i], quality[i], flux[i:i + 1], ferr[i:i + 1], cen[i:i + 1], status=status[:1], sumimage=S[i:i + 1], mask=mask[i:i + 1])
		assert same_bits(got[i], alone[0]), (i, got[i], alone[0])
		dc.check(got[i], oracle_row(times[i], quality[i], flux[i], ferr[i], cen[i], sumimage=S[i], mask=mask[i]), tag=f'T{T} target{i}')


@gpu
@pytest.mark.parametrize('stride', [-1, -70, 1, 69])
def test_refused_strides_write_nothing(ctx, stride):
	times, quality, flux, ferr, cen = small_case()
	Nt, T = flux.shape
	assert stride < T
	lc = _light_curves(ctx, flux, ferr, cen)
	d_time, d_q = ctx.array(times), ctx.array(quality)
	sentinel = np.full((Nt, 10), -12345.0)
	out = ctx.array(sentinel)
	rc = _call(ctx, 'tp_lightcurve_diagnostics_times', Nt, T, lc, d_time, stride, d_q, out)
	assert rc == -1                                                             # TP_ERR_INVALID
	assert b'time stride' in ctx.lib.tp_last_error(ctx.handle)
	ctx.sync()
	assert np.array_equal(out.to_host(), sentinel)
