# -*- coding: utf-8 -*-
"""
The limit cases of tests/halo_limits_common.py show what they claim (no GPU): the sizes and fitted counts named, ties where the
median's cadence is not the first of its equals and a wrong pick changes the gradient by far more than the device test allows,
the float64 restatement's own error at these shapes inside the bound the device is held to, and optimiser runs in which no decision
sits close enough to its threshold for a last-bit difference between the device and numpy to flip it.  Without these a pass of
tests/test_gpu_halo_limits.py would prove nothing.
"""
import numpy as np
import pytest
import halo_common as hc
import halo_limits_common as lc

#: how close (relative to max(|f|, 1)) a decision of the optimiser may sit to its threshold
MARGIN = 1e-9


def test_sizes_and_fitted_counts():
	wide, long_ = lc.wide_cases(), lc.long_cases()
	assert [c.P.shape[1] for c in wide] == [2047, 2048, 2049, 3072, 3073, 4093, 4095, 4096]
	for c in wide:
		ncad = c.P.shape[0]
		assert 65 <= ncad <= 193 and ncad % 64 != 0 and 2 <= -(-ncad // 64) <= 4, c.name
		assert not c.fit[0] and not c.fit[-1] and 3 <= ncad - c.fit.sum() <= 8 and c.fit.sum() == c.nf, c.name
	assert {-(-c.P.shape[0] // 64) % 4 for c in wide} == {0, 2, 3}     # what sum_tiles' chains of four leave over
	assert sorted(c.nf for c in long_) == [20479, 20480, 20481, 21505, 41001]
	assert {c.P.shape[1] for c in long_} == {3, 5, 8}
	for c in long_:
		assert c.fit.sum() == c.nf and c.P.shape[0] > c.nf, c.name
		assert not c.fit[0] and not c.fit[-1] and np.count_nonzero(~c.fit[1:-1]) >= 10, c.name
	# stat_select's re-read loop: none, none, one key, 1025 keys (thread 0 re-reads two), every thread 20 or 21
	assert [max(c.nf - lc.KEYS_CACHED, 0) for c in long_] == [0, 0, 1, 1025, 20521]
	assert {c.nf % 2 for c in long_} == {0, 1}
	for c in wide + long_ + lc.tie_cases():
		assert c.P.dtype == np.float32 and c.fit.dtype == bool and np.all(np.isfinite(c.P)), c.name


def test_every_case_is_non_degenerate():
	for c in lc.wide_cases() + lc.long_cases():
		for th in c.thetas():
			f, g = hc.objective(c.P, c.fit, th)
			assert np.isfinite(f) and f > 0 and np.all(np.isfinite(g)) and np.max(np.abs(g)) > 0, c.name
	for c in lc.tie_cases():
		f, g = hc.objective(c.P, c.fit, np.zeros(8))
		assert np.isfinite(f) and f > 0 and np.max(np.abs(g)) > 0, c.name


def test_no_sign_and_no_median_cadence_is_decided_by_the_last_bit():
	"""
	The sign terms and the median's cadence are discontinuous in l: two fitted neighbours, or two values at the middle ranks, that
	differ by a rounding error of l (some 1e-16 |l| per pixel summed) would make the gradient a matter of the summation order.  At the
	thetas of the objective test -- zero is also where the solver starts -- every such difference is above 1e-12 of the median.
	"""
	for c in lc.wide_cases() + lc.long_cases():
		for th in c.thetas():
			assert lc.sign_margin(c.P, c.fit, th) > 1e-12, (c.name, lc.sign_margin(c.P, c.fit, th))


def test_the_wide_and_long_case():
	c = lc.wide_and_long_case()
	assert c.P.shape == (20490, 4096) and c.fit.sum() == c.nf == 20481 and not c.fit[0] and not c.fit[-1]
	for th in c.thetas():
		f = hc.objective(c.P, c.fit, th, with_grad=False)
		assert np.isfinite(f) and f > 0 and lc.sign_margin(c.P, c.fit, th) > 1e-12


@pytest.mark.parametrize('case', lc.tie_cases(), ids=lambda c: c.name)
def test_ties_put_the_median_among_equals(case):
	P, fit = case.problem
	assert P.shape[1] == 8 and fit.sum() == case.nf
	# exact arithmetic: integer rows of at most three sums, l = sum / 8
	assert np.array_equal(P, np.round(P)) and P.min() >= 0 and P.max() < 2**10
	lF = P[fit].astype('float64') @ hc.softmax(np.zeros(8))
	assert np.array_equal(lF * 8, P[fit].astype('int64').sum(axis=1)) and 2 <= len(np.unique(lF)) <= 3
	for value in np.unique(lF):
		assert len(np.unique(P[fit][lF == value], axis=0)) > 0.9 * np.count_nonzero(lF == value)
	med = lc.median_cadences(case)
	assert tuple(m['shared'] for m in med) == case.expect['shared'], med
	assert tuple(m['occurrence'] for m in med) == case.expect['occurrence'], med
	assert len(med) == 2 - case.nf % 2
	rows = [m['cadence'] for m in med]
	for m in med:
		if m['occurrence'] > 0:
			assert not np.array_equal(P[m['cadence']], P[m['first']]), m
	if len(med) == 2:
		assert not np.array_equal(P[rows[0]], P[rows[1]])
	# the restatement's gradient is the one with these rows, and the first occurrences' rows give another by far more than 1e-10
	f, g = hc.objective(P, fit, np.zeros(8))
	gmax = np.max(np.abs(g))
	assert np.max(np.abs(lc.gradient_with_rows(case, rows) - g)) <= 1e-14 * gmax
	wrong = lc.gradient_with_rows(case, [m['first'] for m in med])
	assert np.max(np.abs(wrong - g)) > 1e-3 * gmax, np.max(np.abs(wrong - g)) / gmax
	if case.name.startswith('tie-second-round'):
		# find_occurrence looks at 1024 fitted cadences per round: the median's lies beyond the first round and has equals before it there
		assert all(m['fitted_index'] >= 1024 and m['occurrence'] >= 1024 for m in med)
	if case.name.endswith('unfitted'):
		assert all(m['cadence'] != m['fitted_index'] for m in med)


def _objective_longdouble(P, fit, theta):
	"""``halo_common.objective``'s f with the same w, every sum in ``np.longdouble``."""
	w = hc.softmax(theta).astype(np.longdouble)
	lF = (P[fit].astype(np.longdouble) * w[None, :]).sum(axis=1)
	return np.sum(np.abs(np.diff(lF))) / np.median(lF)


def test_the_restatement_is_exact_enough_at_these_shapes():
	"""The float64 restatement against itself in longdouble: a small share of the bound the device is held to against it."""
	assert np.finfo(np.longdouble).eps < 1e-18
	worst = (0.0, None)
	for c in lc.wide_cases() + lc.long_cases():
		for th in c.thetas():
			f = hc.objective(c.P, c.fit, th, with_grad=False)
			bound, scale = lc.objective_bound(c.P, c.fit, th, f)
			err = abs(float(_objective_longdouble(c.P, c.fit, th) - np.longdouble(f)))
			assert err <= 0.1 * bound, (c.name, err, bound)
			worst = max(worst, (err / bound, c.name))
	print(f"float64 restatement against longdouble: at most {worst[0]:.3g} of the device bound ({worst[1]})")


@pytest.mark.parametrize('setting', lc.SOLVER_SETTINGS, ids=lc.setting_id)
def test_no_decision_of_the_optimiser_is_marginal(setting):
	"""Every line-search trial, every pair and every ftol test of every solver case keeps MARGIN from its threshold."""
	maxiter, history, ftol, gtol = setting
	for i, c in enumerate(lc.solver_cases()):
		res, trace = lc.reference(i, setting)
		assert res['status'] in (hc.CONVERGED, hc.CAP_REACHED) and res['iterations'] <= maxiter, (c.name, res['status'])
		for fn, threshold, accepted in trace.get('trials', ()):
			assert np.isfinite(fn) and accepted == (fn <= threshold)
			assert abs(fn - threshold) > MARGIN * max(abs(threshold), 1.0), (c.name, fn, threshold)
		scale = max(abs(res['f']), 1.0)
		for sy, curv, kept in trace.get('pairs', ()):
			assert kept == (sy > curv) and abs(sy - curv) > MARGIN * scale, (c.name, sy, curv)
		for drop, tol, gmax in trace.get('stops', ()):
			assert abs(drop - tol) > MARGIN * scale, (c.name, drop, tol)
			assert abs(gmax - gtol) > 1e-6 * gtol, (c.name, gmax)
		assert len(trace.get('pairs', ())) == res['iterations']


def test_the_settings_reach_the_exits_they_name():
	cases = lc.solver_cases()
	runs = {lc.setting_id(s): [lc.reference(i, s) for i in range(len(cases))] for s in lc.SOLVER_SETTINGS}
	stored = lambda trace: sum(kept for _, _, kept in trace.get('pairs', ()))
	assert all(r['iterations'] == 0 and r['status'] == hc.CAP_REACHED for r, _ in runs['maxiter0-history10'])
	assert all(r['iterations'] == 1 and r['status'] == hc.CAP_REACHED for r, _ in runs['maxiter1-history10'])
	assert all(r['iterations'] == 2 and r['status'] == hc.CAP_REACHED for r, _ in runs['maxiter2-history1'])
	assert all(r['iterations'] == 3 and r['status'] == hc.CAP_REACHED for r, _ in runs['maxiter3-history2'])
	assert all(r['iterations'] == 1 and r['status'] == hc.CONVERGED for r, _ in runs['maxiter12-history10-ftol1'])
	assert all(r['iterations'] == 0 and r['status'] == hc.CONVERGED for r, _ in runs['maxiter12-history10-gtol1e30'])
	# a ring of one slot and of two overrun by every wide case and by most long ones; the ring of 16 by every wide case and by two
	# long ones; some long case has a pair the rule rejects
	kinds = [c.kind for c in cases]
	for name, more_than in (('maxiter2-history1', 1), ('maxiter3-history2', 2), ('maxiter12-history1', 8)):
		over = [k for k, (_, t) in zip(kinds, runs[name]) if stored(t) > more_than]
		assert over.count('wide') == len(lc.wide_cases()) and over.count('long') >= 3, (name, over)
	assert any(stored(t) < r['iterations'] for r, t in runs['maxiter12-history10'])
	over = [c.kind for c, (_, t) in zip(cases, runs['maxiter40-history16']) if stored(t) > 16]
	assert over.count('wide') == len(lc.wide_cases()) and over.count('long') >= 2, over
	# the line search halves at least once somewhere, and a history of 1 gives another path than a history of 10
	assert any(len(t['trials']) > r['iterations'] for r, t in runs['maxiter12-history10'])
	assert any(a['f'] != b['f'] for (a, _), (b, _) in zip(runs['maxiter12-history1'], runs['maxiter12-history10']))


def test_trace_changes_nothing():
	c = lc.long_cases()[0]
	plain = hc.lbfgs(c.P, c.fit, maxiter=12)
	traced, _ = lc.reference(len(lc.wide_cases()), (12, 10, hc.FTOL, hc.GTOL))
	assert plain['f'] == traced['f'] and plain['iterations'] == traced['iterations'] and np.array_equal(plain['theta'], traced['theta'])
