# -*- coding: utf-8 -*-
"""
The Halo solver's cases at the size limits its header promises (``1 <= npix <= 4096``, any number of cadences), shared by
tests/test_halo_limits_host.py (the cases show what they claim, no GPU) and tests/test_gpu_halo_limits.py (the device against the
restatement tests/halo_common.py on them).  Every case comes from a fixed seed and has an explicit fit mask, so the number of fitted
cadences ``nf`` -- what the stat kernel's branches depend on -- is exactly the number named.

Which branch of csrc/halo.hip a case reaches:

* wide (``npix`` 2047 .. 4096, 65 .. 193 cadences): a backward thread's float4 column ``k`` is pixel chunk ``threadIdx.x + 256 k``;
  2047 and 2048 pixels end in the last chunk of column 1, 2049 starts column 2, 3072 fills it, 3073 starts column 3, 4093 / 4095 /
  4096 end in its last chunk (with 3, 1 and 0 pixels of padding).  The same sizes are the wide end of every per-pixel loop of the
  finish kernel (8, 9, 12, 13 and 16 rounds of 256 threads) and of the forward kernel's LDS copy of ``w`` (up to 32 KB).  The cadence
  counts are two, three and four 64-cadence tiles with the last one partial: ``sum_tiles``' chains of four leave 2, 3 and 0 over.
* long (``npix`` 3, 5, 8): the stat kernel caches 20 * 1024 = 20 480 keys of the fitted light curve in registers and ``stat_select``
  re-reads the rest: ``nf`` = 20 479 and 20 480 stay inside the cache, 20 481 re-reads one key, 21 505 = 20 480 + 1 025 gives one
  thread two keys to re-read, 41 001 gives every thread 20 or 21.
* wide and long (4096 pixels, ``nf`` = 20 481): both at once, objective only.
* ties (8 pixels, small integer rows, evaluated at ``theta = 0`` where ``w = 1/8`` exactly): every ``l_t`` is an exact multiple of
  1/8 on both sides, many cadences share the median's key, and ``find_occurrence`` has to pick the right one of them: the gradient's
  median term is that cadence's row.

The solver settings run on the wide and long cases reach the exits after 0, 1, 2 and 3 iterations, a history ring of 1 slot and one
of 16 slots overrun (more than 16 pairs stored in 40 iterations), and both tolerance exits.
"""
import functools
import numpy as np
import halo_common as hc

#: (npix, ncad): two to four 64-cadence tiles, the last one partial
WIDE = ((2047, 65), (2048, 129), (2049, 66), (3072, 130), (3073, 193), (4093, 100), (4095, 67), (4096, 191))
#: (npix, nf, ncad)
LONG = ((3, 20479, 20523), (5, 20480, 20531), (8, 20481, 20527), (5, 21505, 21560), (3, 41001, 41064))
WIDE_AND_LONG = (4096, 20481, 20490)
KEYS_CACHED = 20 * 1024

#: (maxiter, history, ftol, gtol)
SOLVER_SETTINGS = (
	(0, 10, hc.FTOL, hc.GTOL),
	(1, 10, hc.FTOL, hc.GTOL),
	(2, 1, hc.FTOL, hc.GTOL),
	(3, 2, hc.FTOL, hc.GTOL),
	(12, 1, hc.FTOL, hc.GTOL),
	(12, 10, hc.FTOL, hc.GTOL),
	(40, 16, hc.FTOL, hc.GTOL),     # more than 16 pairs: the ring of 16 slots is overrun
	(12, 10, 1.0, hc.GTOL),         # ftol: f_k - f_k+1 <= max(|f_k|, |f_k+1|, 1) holds after the first iteration -> status 1
	(12, 10, hc.FTOL, 1e30),        # gtol: the first gradient is below it -> 0 iterations, status 1
)


def setting_id(s):
	return f'maxiter{s[0]}-history{s[1]}' + ('-ftol1' if s[2] != hc.FTOL else '') + ('-gtol1e30' if s[3] != hc.GTOL else '')


class Case(object):
	"""``P`` float32 (ncad, npix), ``fit`` bool (ncad,), ``name``, ``kind`` ('wide', 'long', 'wide_and_long', 'tie'), ``nf`` named."""
	def __init__(self, name, kind, P, fit, nf, **expect):
		self.name, self.kind, self.P, self.fit, self.nf, self.expect = name, kind, P, fit, nf, expect

	@property
	def problem(self):
		return (self.P, self.fit)

	def thetas(self):
		"""The two points the objective is compared at: zero, and ``normal * 0.5``."""
		npix = self.P.shape[1]
		seed = npix * 100003 + self.P.shape[0]
		return [np.zeros(npix), np.random.default_rng(seed).normal(size=npix) * 0.5]


def _pixels(npix, ncad, seed):
	"""The pixel values of ``_problem`` (tests/test_gpu_halo.py): a slow sinusoid, a random walk seen differently by every pixel, noise."""
	rng = np.random.default_rng(seed)
	base = rng.uniform(50, 1000, npix)
	walk = np.cumsum(rng.normal(size=ncad)) * 0.01
	P = base[None, :] * (1 + 1e-3 * np.sin(np.arange(ncad) / 7.0))[:, None] * (1 + 0.05 * walk[:, None] * rng.normal(size=npix)[None, :])
	return (P + rng.normal(size=(ncad, npix)) * 2).astype('float32'), rng


def _fit_mask(ncad, nf, rng):
	"""``ncad - nf`` cadences unfitted: the first and the last two, the others scattered."""
	n_out = ncad - nf
	assert n_out >= 4
	fit = np.ones(ncad, dtype=bool)
	fit[[0, ncad - 2, ncad - 1]] = False
	fit[1 + rng.choice(ncad - 4, size=n_out - 3, replace=False)] = False
	return fit


def _long_pixels(npix, ncad, seed):
	"""
	Few pixels over many cadences: a random walk of 1e-5 per cadence that the pixels see with coefficients of both signs (so weights
	exist that cancel it) and noise of 3e-4 on fluxes of 50 .. 1000.  f is of the order of 0.01, as in the wide cases: a
	long case with the noise of ``_pixels`` would converge within twenty iterations, where every decision of the line search is
	marginal by nature (the last accepted step lowers f by less than ``ftol``).
	"""
	rng = np.random.default_rng(seed)
	base = rng.uniform(50, 1000, npix)
	walk = np.cumsum(rng.normal(size=ncad)) * 1e-5
	a = rng.normal(size=npix)
	a[0], a[1] = abs(a[0]) + 0.5, -abs(a[1]) - 0.5
	P = base[None, :] * (1 + walk[:, None] * a[None, :])
	return (P + rng.normal(size=(ncad, npix)) * 3e-4).astype('float32'), rng


#: seeds: one that leaves a decision of the optimiser within 1e-9 of its threshold (tests/test_halo_limits_host.py) is replaced here
#: (long cases: of the seeds 1 .. 8 tried per case these are the first that keep the margin under every setting)
WIDE_SEEDS = {2047: 2047, 2048: 2048, 2049: 2049, 3072: 3072, 3073: 3073, 4093: 4093, 4095: 4095, 4096: 4096}
LONG_SEEDS = {20479: 1, 20480: 1, 20481: 2, 21505: 1, 41001: 2}


@functools.lru_cache(maxsize=None)
def wide_cases():
	out = []
	for npix, ncad in WIDE:
		P, rng = _pixels(npix, ncad, WIDE_SEEDS[npix])
		fit = _fit_mask(ncad, ncad - 5, rng)
		out.append(Case(f'wide-{npix}x{ncad}', 'wide', P, fit, ncad - 5))
	return tuple(out)


def _separate(P, fit):
	"""
	With equal weights (``theta = 0``, where the solver starts) ``l`` is the plain sum of a cadence's few float32 pixel values, and with
	noise of ten float32 steps consecutive cadences tie by chance (about one pair in sixty).  A tie is a sign term ``s_t`` that the last
	bit of ``l`` decides, on the device and in numpy alike: pixel 0 of the later cadence moves up by one float32 step until no two
	consecutive fitted cadences, and none of the values round the middle ranks, have the same sum (exact in float64).
	"""
	F = np.flatnonzero(fit)
	nf = len(F)
	for _ in range(1000):
		total = P[F].astype('float64').sum(axis=1)
		rows = set((np.flatnonzero(np.diff(total) == 0) + 1).tolist())
		order = np.argsort(total, kind='stable')
		for k in range((nf - 1) // 2 - 1, nf // 2 + 1):
			if total[order[k]] == total[order[k + 1]]:
				rows.add(int(order[k + 1]))
		if not rows:
			return P
		rows = F[sorted(rows)]
		P[rows, 0] = np.nextafter(P[rows, 0], np.float32(np.inf))
	raise AssertionError('ties left')


def _long_case(npix, nf, ncad, seed):
	P, rng = _long_pixels(npix, ncad, seed)
	fit = _fit_mask(ncad, nf, rng)
	return Case(f'long-{npix}x{nf}', 'long', _separate(P, fit), fit, nf)


@functools.lru_cache(maxsize=None)
def long_cases():
	return tuple(_long_case(npix, nf, ncad, LONG_SEEDS[nf]) for npix, nf, ncad in LONG)


def sign_margin(P, fit, theta):
	"""
	How far the signs and the median's cadence are from a tie at ``theta``, relative to the median: the smallest ``|l_j+1 - l_j|`` over
	the fitted cadences, and the smallest gap between the values of the ranks next to and at the middle.
	"""
	lF = P[fit].astype('float64') @ hc.softmax(theta)
	nf = len(lF)
	srt = np.sort(lF)
	middle = np.diff(srt[(nf - 1) // 2 - 1:nf // 2 + 2])
	if nf % 2 == 0:
		middle = np.delete(middle, 1)      # (the two middle values may be equal: both rows enter the median term either way)
	return min(np.min(np.abs(np.diff(lF))), np.min(middle)) / np.median(lF)


def wide_and_long_case():
	"""4096 pixels, 20 481 fitted cadences (a 336 MB ``P``; the noise drawn in float32 to build it quickly).  Not cached."""
	npix, nf, ncad = WIDE_AND_LONG
	rng = np.random.default_rng(7)
	base = rng.uniform(50, 1000, npix).astype('float32')
	walk = (np.cumsum(rng.normal(size=ncad)) * 0.01).astype('float32')
	P = rng.standard_normal(size=(ncad, npix), dtype='float32')
	P *= 2
	P += base[None, :] * (1 + np.float32(0.05) * walk[:, None])
	return Case(f'wide-and-long-{npix}x{nf}', 'wide_and_long', P, _fit_mask(ncad, nf, rng), nf)


def solver_cases():
	"""The cases the short solver runs go over: every wide and every long one."""
	return wide_cases() + long_cases()


# -- ties -------------------------------------------------------------------------------------------------------------------------
def _tie_case(name, seed, sums, counts, unfitted=0, **expect):
	"""
	8 pixels; ``counts[i]`` fitted cadences whose row sums to ``sums[i]`` (so ``l = sums[i] / 8`` exactly at ``theta = 0``), shuffled in
	time; every row is its own draw ``multinomial(sum - 160, 1/8) + 20``, so rows of one sum hold different pixel values.
	``unfitted`` cadences of the same kind are scattered in between (and put first and last).
	"""
	rng = np.random.default_rng(seed)
	nf = int(np.sum(counts))
	level = rng.permutation(np.repeat(np.arange(len(sums)), counts))
	ncad = nf + unfitted
	fit = np.ones(ncad, dtype=bool)
	if unfitted:
		fit[[0, ncad - 1]] = False
		fit[1 + rng.choice(ncad - 2, size=unfitted - 2, replace=False)] = False
	row_sum = np.empty(ncad, dtype='int64')
	row_sum[fit] = np.asarray(sums)[level]
	row_sum[~fit] = rng.choice(sums, size=unfitted)
	P = np.stack([rng.multinomial(s - 160, np.ones(8) / 8) + 20 for s in row_sum]).astype('float32')
	return Case(name, 'tie', P, fit, nf, **expect)


@functools.lru_cache(maxsize=None)
def tie_cases():
	"""
	``shared``: how many fitted cadences share the key of each middle rank; ``occurrence``: the index of each median cadence among
	the fitted cadences of its key, in time order -- both follow from the counts: the ranks below a key are the counts of the
	smaller sums.
	"""
	sums = (400, 408, 424)
	return (
		# odd nf: rank 500 is occurrence 500 - 300 of the middle sum
		_tie_case('tie-odd', 11, sums, (300, 500, 201), shared=(500,), occurrence=(200,)),
		# even nf, ranks 766 and 767 both in the middle sum: occurrences 466 and 467
		_tie_case('tie-even-inside', 12, sums, (300, 900, 334), shared=(900, 900), occurrence=(466, 467)),
		# even nf, rank 499 the last of the first sum, rank 500 the first of the second
		_tie_case('tie-even-straddling', 13, sums, (500, 300, 200), shared=(500, 300), occurrence=(499, 0)),
		# two sums, nf 5001: rank 2500 is occurrence 1250 of the larger sum -- find_occurrence counts 1024 candidates per round
		_tie_case('tie-second-round', 14, sums[:2], (1250, 3751), shared=(3751,), occurrence=(1250,)),
		# the same, even, with 700 unfitted cadences in between: the cadence index is not the fitted index
		_tie_case('tie-second-round-unfitted', 15, sums[:2], (1250, 3750), unfitted=700, shared=(3750, 3750), occurrence=(1249, 1250)),
	)


def median_cadences(case, theta=None):
	"""
	The cadence (index into the problem) of each middle rank of the fitted light curve in the stable order, how many fitted cadences
	share its value, its occurrence index among them in time order, and the cadence of that value's first occurrence.
	"""
	P, fit = case.problem
	F = np.flatnonzero(fit)
	w = hc.softmax(np.zeros(P.shape[1]) if theta is None else theta)
	lF = P[F].astype('float64') @ w
	order = np.argsort(lF, kind='stable')
	nf = len(F)
	out = []
	for k in sorted({(nf - 1) // 2, nf // 2}):
		j = order[k]
		same = np.flatnonzero(lF == lF[j])
		out.append({'cadence': int(F[j]), 'fitted_index': int(j), 'shared': len(same), 'occurrence': int(np.searchsorted(same, j)),
			'first': int(F[same[0]])})
	return out


def gradient_with_rows(case, rows):
	"""``halo_common.objective``'s gradient at ``theta = 0`` with the median term taken from the cadences ``rows`` (mean of two)."""
	P, fit = case.problem
	F = np.flatnonzero(fit)
	npix = P.shape[1]
	w = hc.softmax(np.zeros(npix))
	PF = P[F].astype('float64')
	lF = PF @ w
	m = np.median(lF)
	dl = np.diff(lF)
	f = np.sum(np.abs(dl)) / m
	sg = np.sign(dl)
	s = np.zeros(len(F))
	s[1:] += sg
	s[:-1] -= sg
	pm = np.mean([P[r].astype('float64') for r in rows], axis=0)
	g = (s @ PF) / m - (f / m) * pm
	return w * (g - w @ g)


# -- the restatement, once per case and setting -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(index, setting):
	"""``halo_common.lbfgs`` on solver case ``index`` under ``setting``, with its trace: ``(result, trace)``.  Computed once."""
	case = solver_cases()[index]
	maxiter, history, ftol, gtol = setting
	trace = {}
	res = hc.lbfgs(case.P, case.fit, maxiter=maxiter, history=history, ftol=ftol, gtol=gtol, trace=trace)
	return res, trace


def objective_bound(P, fit, theta, fr):
	"""The bound of ``test_objective_against_the_restatement`` on ``|df|``: ``1e-12 |f| + 1e-14 sum_j (|l_j| + |l_j+1|) / m``."""
	lF = P[fit].astype('float64') @ hc.softmax(theta)
	scale = np.sum(np.abs(lF[1:]) + np.abs(lF[:-1])) / np.median(lF)
	return 1e-12 * abs(fr) + 1e-14 * scale, scale
