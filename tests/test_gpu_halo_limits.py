# -*- coding: utf-8 -*-
"""
The Halo kernels (csrc/halo.hip) against the restatement (tests/halo_common.py) at the size limits the header promises: 2047 .. 4096
pixels (float4 columns 2 and 3 of the backward kernel, the wide end of the finish kernel's loops, the 32 KB of ``w`` in the forward
kernel's LDS), 20 479 .. 41 001 fitted cadences (the keys ``stat_select`` re-reads beyond the 20 480 it caches), medians among equal
values (``find_occurrence`` with a rank above zero, and above 1024: its second round), and optimiser settings the device had not
run: history 1, 2 and 16, ``maxiter`` 0 .. 3, 12 and 40, both tolerance exits.  The cases and what each reaches are
tests/halo_limits_common.py; tests/test_halo_limits_host.py shows, without a GPU, that they are what they claim.
"""
import numpy as np
import pytest
import halo_common as hc
import halo_limits_common as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _hold_objective(ctx, cases, label):
	"""``halo.objective`` on every case at its two thetas in one call, under the bound of ``test_objective_against_the_restatement``."""
	from photometry_amd import halo
	probs, thetas, names = [], [], []
	for c in cases:
		for th in c.thetas():
			probs.append(c.problem)
			thetas.append(th)
			names.append(c.name)
	f, grads = halo.objective(ctx, probs, thetas)
	bad, worst_f, worst_g = [], 0.0, 0.0
	for i, ((P, fit), th) in enumerate(zip(probs, thetas)):
		fr, gr = hc.objective(P, fit, th)
		assert np.isfinite(fr), names[i]
		bound, scale = lc.objective_bound(P, fit, th, fr)
		ef = abs(f[i] - fr)
		dg, gmax = np.max(np.abs(grads[i] - gr)), np.max(np.abs(gr))
		worst_f = max(worst_f, ef / bound)
		worst_g = max(worst_g, dg / gmax)
		print(f"{names[i]:28s} |df| / |f| {ef / abs(fr):.2e}  |df| / bound {ef / bound:.3f}  |dg|_inf / |g|_inf {dg / gmax:.2e}")
		if not (ef <= bound and dg <= 1e-10 * gmax):
			bad.append((names[i], ef / abs(fr), ef / scale, dg / gmax))
	print(f"{label}: worst |df| {worst_f:.3f} of the bound, worst gradient (relative to |grad|_inf) {worst_g:.2e}")
	assert not bad, bad


def test_objective_at_the_limits(ctx):
	"""Measured on one MI355X: see DESIGN.md section 10 ("Parity at the size limits")."""
	_hold_objective(ctx, lc.wide_cases() + lc.long_cases(), 'objective, wide and long')


def test_objective_wide_and_long(ctx):
	_hold_objective(ctx, [lc.wide_and_long_case()], 'objective, wide and long at once')


def test_ties(ctx):
	"""At ``theta = 0`` every operand of f is exact on both sides: f bit for bit; the gradient within 1e-10 of ``|grad|_inf`` -- a wrong
	occurrence of the median's key is off by more than 1e-3 (tests/test_halo_limits_host.py)."""
	from photometry_amd import halo
	cases = lc.tie_cases()
	f, grads = halo.objective(ctx, [c.problem for c in cases], [np.zeros(8) for _ in cases])
	for i, c in enumerate(cases):
		fr, gr = hc.objective(c.P, c.fit, np.zeros(8))
		dg = np.max(np.abs(grads[i] - gr)) / np.max(np.abs(gr))
		print(f"{c.name:28s} f {f[i]!r} (restatement {fr!r})  |dg|_inf / |g|_inf {dg:.2e}")
		assert f[i] == fr, (c.name, f[i], fr)
		assert dg <= 1e-10, (c.name, dg)


#: |f_dev / f_ref - 1| and max |dw| allowed per setting: ten times the worst over all wide and long cases measured on one MI355X,
#: rounded up (the device orders its float64 sums differently from numpy, and how much that moves a trajectory varies with the data),
#: never looser than the project's allowances 1e-6 and 1e-6.  The measured worst stands behind each; where the weights came out equal
#: bit for bit (no iteration: softmax(0)) the allowance is one rounding of a weight.
SOLVER_BOUNDS = {
	'maxiter0-history10': (8.3e-12, 1e-15),            # measured 8.28e-13, 0
	'maxiter1-history10': (1.1e-10, 9.5e-14),          # measured 1.02e-11, 9.49e-15
	'maxiter2-history1': (3.1e-11, 9.3e-14),           # measured 3.06e-12, 9.24e-15
	'maxiter3-history2': (7.1e-11, 9.2e-14),           # measured 7.06e-12, 9.19e-15
	'maxiter12-history1': (1.6e-10, 9.2e-11),          # measured 1.52e-11, 9.20e-12
	'maxiter12-history10': (1.5e-10, 1.2e-10),         # measured 1.49e-11, 1.11e-11
	'maxiter40-history16': (5.9e-11, 2.4e-8),          # measured 5.86e-12, 2.34e-9
	'maxiter12-history10-ftol1': (1.1e-10, 9.5e-14),   # measured 1.02e-11, 9.49e-15
	'maxiter12-history10-gtol1e30': (8.3e-12, 1e-15),  # measured 8.28e-13, 0
}


@pytest.mark.parametrize('setting', lc.SOLVER_SETTINGS, ids=lc.setting_id)
def test_short_solver_runs(ctx, setting):
	from photometry_amd import halo
	cases = lc.solver_cases()
	maxiter, history, ftol, gtol = setting
	dev = halo.tvmin(ctx, [c.problem for c in cases], maxiter=maxiter, history=history, ftol=ftol, gtol=gtol)
	worst_f = worst_w = 0.0
	for i, c in enumerate(cases):
		ref, _ = lc.reference(i, setting)
		where = (c.name, int(dev['status'][i]), ref['status'], int(dev['iterations'][i]), ref['iterations'])
		assert dev['status'][i] == ref['status'] and dev['iterations'][i] == ref['iterations'], where
		assert np.all(dev['w'][i] >= 0) and abs(np.sum(dev['w'][i]) - 1) < 1e-12, c.name
		lcurve, _ = hc.light_curve(c.P, c.fit, dev['w'][i])
		np.testing.assert_allclose(dev['l'][i], lcurve, rtol=1e-12, err_msg=c.name)
		assert dev['f'][i] <= ref['f'] * (1 + 1e-6), (c.name, dev['f'][i], ref['f'])
		df, dw = abs(dev['f'][i] / ref['f'] - 1), np.max(np.abs(dev['w'][i] - ref['w']))
		assert dw <= 1e-6, (c.name, dw)
		print(f"{lc.setting_id(setting):28s} {c.name:16s} iterations {ref['iterations']:2d} status {ref['status']}  |f_dev / f_ref - 1| {df:.2e}  max |dw| {dw:.2e}")
		worst_f, worst_w = max(worst_f, df), max(worst_w, dw)
	print(f"{lc.setting_id(setting)}: worst |f_dev / f_ref - 1| {worst_f:.2e}, worst max |dw| {worst_w:.2e}")
	bound_f, bound_w = SOLVER_BOUNDS[lc.setting_id(setting)]
	assert bound_f <= 1e-6 and bound_w <= 1e-6
	assert worst_f <= bound_f and worst_w <= bound_w, (worst_f, bound_f, worst_w, bound_w)


def test_same_bits_alone_in_a_batch_and_twice(ctx):
	"""``test_bit_reproducible_and_batch_independent`` at the limits: the cases in another order, and three of them alone."""
	from photometry_amd import halo
	cases = lc.wide_cases() + lc.long_cases() + lc.tie_cases()
	run = lambda cs: halo.tvmin(ctx, [c.problem for c in cs], maxiter=12)
	batch = run(cases)
	order = list(range(len(cases)))[::-1]
	order = order[1::2] + order[::2]
	other = run([cases[i] for i in order])

	def same(a, j, i, label):
		assert np.array_equal(a['w'][j], batch['w'][i]) and np.array_equal(a['l'][j], batch['l'][i]), (label, cases[i].name)
		assert np.array_equal(a['f'][j:j + 1], batch['f'][i:i + 1], equal_nan=True), (label, cases[i].name)
		assert a['iterations'][j] == batch['iterations'][i] and a['status'][j] == batch['status'][i], (label, cases[i].name)
	for j, i in enumerate(order):
		same(other, j, i, 'another order')
	names = [c.name for c in cases]
	for name in ('wide-4096x191', 'long-5x21505', 'tie-second-round-unfitted'):
		i = names.index(name)
		same(run([cases[i]]), 0, i, 'alone')
	assert np.all(batch['status'] != hc.DEGENERATE)
