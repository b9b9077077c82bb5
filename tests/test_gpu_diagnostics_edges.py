# -*- coding: utf-8 -*-
"""
``tp_lightcurve_diagnostics`` against the oracle where one seeded generator (tests/test_gpu_diagnostics.py) never takes it: the
radix select on negative, tied, infinite, signed-zero and subnormal keys; 0..5 good cadences through a per-target quality and a
non-default bitmask; samples on the edges of numpy's ``arange`` / ``searchsorted(right)`` bins, duplicate, NaN, infinite and
unsorted time stamps; both sides of the dense / sparse binning switch; fluxes whose median is negative or zero; a pitched
light-curve block; both sides of the LDS / HBM switch of the series arrays.  The cases are built in tests/diagnostics_common.py
and their oracle rows are pinned by known answers in tests/test_oracle_diagnostics_edges.py.

Every case is held to ``oracle.diagnostics.diagnostics`` column by column, flags included, with the tolerances of
tests/test_gpu_diagnostics.py (exact medians, mask_size and edge_flux; 1e-12 variance and rms_hour; 1e-9 variability).
"""
import ctypes
import numpy as np
import pytest
import diagnostics_common as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def against_oracle(ctx, case, tag, **check_kwargs):
	time, quality, flux, ferr, cen, kwargs = case
	got = dc.run(ctx, time, quality, flux, ferr, cen, **kwargs)
	ref = dc.oracle_rows(*case)
	for i in range(len(flux)):
		dc.check(got[i], ref[i], tag=f'{tag} target{i}', **check_kwargs)
	return got, ref


# ---- a. selection
@pytest.mark.parametrize('T', [255, 256, 257])
def test_selection(ctx, T):
	"""block_median on both sides of the workgroup width: every median of every target equal to numpy's, signed zeros by ``==``."""
	case = dc.selection_case(T)
	time, quality, flux, ferr, cen, kwargs = case
	got = dc.run(ctx, time, quality, flux, ferr, cen)
	ref = dc.oracle_rows(*case)
	from photometry_amd.engine import DIAGNOSTICS_COLUMNS as COLS
	for i, name in enumerate(dc.SELECTION_TARGETS):
		for key in ('mean_flux', 'ptp', 'pos_centroid_col', 'pos_centroid_row'): # first the medians alone: the message names the target
			g, r = got[i][COLS.index(key)], ref[i][key]
			assert g == r or (np.isnan(g) and np.isnan(r)), (T, name, key, g, r)
		dc.check(got[i], ref[i], tag=f'T{T} {name}')


# ---- b. few good cadences
@pytest.mark.parametrize('bitmask', [dc.DEFAULT_BITMASK, 16])
def test_few_good_cadences(ctx, bitmask):
	"""0..5 good cadences per target through a 2-D quality (``quality_target_stride != 0``), under the default bitmask and under
	``bitmask = 16``.  With at most 4 fitted cadences the cubic is exact or undefined and ``variability`` is rounding noise over a
	number: there ``|got - ref| <= 1e-9 * nanstd(rel) / nanmedian(rel_err)``, the project's 1e-9 on the undetrended scale."""
	case = dc.few_good_case(bitmask)
	time, quality, flux, ferr, cen, kwargs = case
	got = dc.run(ctx, time, quality, flux, ferr, cen, **kwargs)
	ref = dc.oracle_rows(*case)
	for i in range(len(flux)):
		few = dc.fitted_cadences(time, quality, flux, ferr, i, kwargs) <= 4
		atol = 1e-9 * dc.undetrended_scale(quality, flux, ferr, i, kwargs) if few else None
		if few and not (atol >= 0): # no good cadence, or none with a flux: the variability is NaN on both sides
			atol = 0.0
		dc.check(got[i], ref[i], tag=f'bitmask {bitmask} target{i} ({dc.few_good_counts(bitmask)[i]} good)', variability_atol=atol)


# ---- c. time axis
@pytest.mark.parametrize('name', [n for n in dc.TIME_CASES if n != 'bins257_permuted'])
def test_time_axis(ctx, name):
	"""Samples on bin edges (exact and rounded ``delta``), duplicate / NaN / infinite / three distinct time stamps, a permuted series
	(the unsorted dense path) and 256 / 257 bins at 200 cadences (both sides of the dense / sparse switch)."""
	against_oracle(ctx, dc.time_case(name), name)


def test_too_many_bins_unsorted(ctx):
	"""257 one-hour bins, more than the kernel's bin array (256 entries at up to 256 cadences), on a series that is NOT in time order:
	the kernel's sparse path needs the samples of a bin to be a contiguous run, so it gives up with flag 16 and ``rms_hour = NaN``.
	This is the kernel's documented limit, not the reference's behaviour (the oracle returns a number and no flag); every other
	column still equals the oracle."""
	case = dc.time_case('bins257_permuted')
	time, quality, flux, ferr, cen, kwargs = case
	assert dc.n_bins(time, quality, kwargs) == 257
	got = dc.run(ctx, time, quality, flux, ferr, cen, **kwargs)
	ref = dc.oracle_rows(*case)
	from photometry_amd.engine import DIAGNOSTICS_COLUMNS as COLS
	for i in range(len(flux)):
		assert int(got[i][COLS.index('flags')]) == 16 and ref[i]['flags'] == 0 and np.isfinite(ref[i]['rms_hour'])
		assert np.isnan(got[i][COLS.index('rms_hour')])
		dc.check(got[i], ref[i], tag=f'target{i}', skip=('rms_hour', 'flags'))


# ---- d. degenerate flux
def test_degenerate_flux(ctx):
	"""Median flux < 0, exactly 0 with non-zero samples (no finite relative flux: BAD_TIME | NO_DETREND as for the reference's
	ValueError out of ``binned_statistic``), all-zero flux, one infinite sample."""
	against_oracle(ctx, dc.degenerate_case(), 'degenerate')


# ---- e. layout
def test_pitched_block_and_error_status(ctx):
	"""The C ABI with ``lc_pitch = n_cad + 7``, the padding filled with 1e30 (finite: a read of it moves a median), and an ERROR target
	between two OK ones: bit for bit the packed call, the ERROR row all NaN."""
	rng = np.random.default_rng(31)
	Nt, T, pad = 3, 257, 7
	time = dc.jittered_time(rng, T)
	quality = np.zeros((Nt, T), dtype='int32')
	quality[rng.random((Nt, T)) < 0.05] = 32
	flux, ferr, cen = dc.ordinary(rng, Nt, T)
	flux[0, 11] = np.nan
	status = np.array([1, 2, 3], dtype='int32') # OK, ERROR, WARNING
	packed = dc.run(ctx, time, quality, flux, ferr, cen, status=status)
	block = np.full((4, Nt, T + pad), 1e30)
	block[0, :, :T], block[1, :, :T], block[2, :, :T], block[3, :, :T] = flux, ferr, cen[..., 0], cen[..., 1]
	d_block, d_time, d_q, d_st = ctx.array(block), ctx.array(time), ctx.array(quality), ctx.array(status)
	out = ctx.empty((Nt, 10), 'float64')
	plane = Nt * (T + pad) * 8
	ctx._check(ctx.lib.tp_lightcurve_diagnostics(ctx.handle, Nt, T, d_block.ptr, d_block.ptr + plane, d_block.ptr + 2 * plane, d_block.ptr + 3 * plane,
		T + pad, d_time.ptr, d_q.ptr, T, dc.DEFAULT_BITMASK, d_st.ptr, None, None, 0, 0, ctypes.c_double(dc.HOUR), out.ptr))
	ctx.sync()
	pitched = out.to_host()
	assert np.all(np.isnan(pitched[1])) and np.all(np.isnan(packed[1]))
	assert np.array_equal(pitched[[0, 2]].view('uint64'), packed[[0, 2]].view('uint64')), (pitched, packed)
	ref = dc.oracle_rows(time, quality, flux, ferr, cen, {})
	for i in (0, 2):
		dc.check(pitched[i], ref[i], tag=f'pitched target{i}')


# ---- f. scratch boundary
@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('side', ['lds', 'hbm'])
def test_scratch_boundary(ctx, side, with_mask):
	"""The largest ``n_cad`` whose series arrays still fit the 160 KiB of LDS and the next one, whose arrays move to HBM scratch
	(sizes from the host formula restated in diagnostics_common.lds_boundary), with and without a 9 x 13 stamp."""
	T = dc.lds_boundary(9, 13) + (side == 'hbm')
	assert T == dc.lds_boundary() + (side == 'hbm') # the stamp's perimeter does not move the boundary
	time, quality, flux, ferr, cen, kwargs, S, mask = dc.boundary_case(T)
	extra = {'sumimage': S, 'mask': mask} if with_mask else {}
	got = dc.run(ctx, time, quality, flux, ferr, cen, status=np.ones(len(flux), dtype='int32'), **extra)
	ref = dc.oracle_rows(time, quality, flux, ferr, cen, kwargs, **extra)
	for i in range(len(flux)):
		dc.check(got[i], ref[i], tag=f'T{T} ({side}) target{i}')
