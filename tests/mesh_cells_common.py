# -*- coding: utf-8 -*-
"""
Designed cells for the mesh statistics kernel (``tp_bkg_mesh_kernel``, csrc/fullframe.hip): the case table of
tests/test_gpu_mesh_cells.py, the mosaic that lays the cells into frames, and the references -- ``oracle.backgrounds.stamp_mask``
and ``mesh_statistics`` alone, never the library.  tests/test_mesh_cells_host.py holds the table to what the names of its cases
promise without a GPU.

A :class:`Case` is one cell: ``box * box`` float32 values, optionally a per-pixel exclude flag and a per-pixel value to subtract.
The pixel mask is taken on the raw values; the statistics run over ``float32(float64(value) - float64(subtract))``
(``layout_common.mesh_expected``).  Inside its cell a case is scrambled by a fixed permutation (:func:`scramble`), so that masked
pixels and extremes are spread over the kernel's four wavefronts and every stride of its sorting network carries work; the cases
whose point is the order of the input (``scramble=False``) are laid out as they are, value ``e`` at row ``e // box``, column
``e % box`` of the cell.

Without the exclude and subtract images (``aux=False``) the same frames are a second, different table: excluded pixels count, keys
are the raw values.  Both tables are held to the same conditions.
"""
import numpy as np

FLUX_CUTOFF = 8e4
F32 = np.float32
#: how a pixel can be masked (backgrounds.py:89-97); 'excluded' needs the exclude image, its pixel holds a valid value
MASK_KINDS = ('nan', '+inf', '-inf', 'negative', 'above', 'excluded')
_MASK_VALUE = {'nan': np.nan, '+inf': np.inf, '-inf': -np.inf, 'negative': -5.0, 'above': 9e4, 'excluded': 100.0}
MAX_ROWS, MAX_COLS = 256, 512          # the largest mosaic frame


class Case(object):
	"""
	One cell.  ``expect``: what the name promises, checked against the oracle in tests/test_mesh_cells_host.py -- ``passes`` (number
	of clipping passes that removed something), ``sides`` (subset of {'top', 'bottom'} clipped over all passes), ``branch`` ('mean':
	std == 0; 'mode': 2.5 med - 1.5 mean; 'median'; 'nan': no valid pixel), ``n`` (valid pixels), ``nmasked``.  ``exact``: every sum
	is exact on both sides by construction; the device is compared with ``==``.
	"""

	def __init__(self, name, box, values, exclude=None, subtract=None, scramble=True, exact=False, **expect):
		self.name, self.box = name, int(box)
		npix = self.box * self.box
		self.values = np.asarray(values, dtype='float32')
		assert self.values.shape == (npix,), (name, self.values.shape)
		self.exclude = None if exclude is None else np.asarray(exclude, dtype=bool)
		self.subtract = None if subtract is None else np.broadcast_to(np.asarray(subtract, dtype='float32'), (npix,)).copy()
		self.scramble, self.exact, self.expect = scramble, exact, expect

	def __repr__(self):
		return f'Case({self.name!r}, box={self.box})'

	def cell(self):
		"""``(values float32, exclude bool, subtract float32)`` as ``(box, box)`` images, in the order they have in the frame."""
		p = scramble(self.box) if self.scramble else np.arange(self.box * self.box)
		shape = (self.box, self.box)
		ex = np.zeros(shape, dtype=bool) if self.exclude is None else self.exclude[p].reshape(shape)
		sub = np.zeros(shape, dtype='float32') if self.subtract is None else self.subtract[p].reshape(shape)
		return self.values[p].reshape(shape), ex, sub


def scramble(box):
	"""The fixed permutation of a cell's ``box * box`` pixels."""
	return np.random.default_rng(1000 + box).permutation(box * box)


def keys_and_mask(case, aux=True):
	"""``(img float32 (box, box), mask bool)``: what the statistics run over, and the pixels they leave out."""
	from oracle import backgrounds as ob
	v, ex, sub = case.cell()
	mask = ob.stamp_mask(v, FLUX_CUTOFF, ex if aux else None)
	img = (v.astype('float64') - sub.astype('float64')).astype('float32') if aux else v
	return img, mask


def expected(cases, aux=True):
	"""``(mesh float64 (n,), nmasked int64 (n,))`` of the oracle, cell by cell."""
	from oracle import backgrounds as ob
	mesh, nm = np.empty(len(cases)), np.empty(len(cases), dtype='int64')
	for k, case in enumerate(cases):
		img, mask = keys_and_mask(case, aux)
		m, n = ob.mesh_statistics(img, mask, box=case.box)
		mesh[k], nm[k] = m[0, 0], n[0, 0]
	return mesh, nm


class Mosaic(object):
	"""The cells of one box size in a stack of frames: ``frames`` float32, ``exclude`` uint8, ``subtract`` float32, all ``(T, R, C)``;
	``cases[k]`` sits in frame ``slots[k][0]`` at mesh row ``slots[k][1]``, mesh column ``slots[k][2]``."""

	def __init__(self, cases, box):
		assert all(c.box == box for c in cases) and len(cases) > 0
		ncol = max(2, min(MAX_COLS // box, -(-len(cases) // 2)))
		rows_max = max(2, MAX_ROWS // box)
		T = -(-len(cases) // (ncol * rows_max))
		nrow = max(2, -(-len(cases) // (T * ncol)))
		cases = list(cases)
		for k in range(len(cases), T * nrow * ncol):           # the slots left over: a constant cell each
			cases.append(Case(f'filler_{k}', box, np.full(box * box, 1.0 + k), exact=True, passes=0, branch='mean'))
		self.box, self.cases, self.shape = box, cases, (T, nrow * box, ncol * box)
		self.mesh_shape = (T, nrow, ncol)
		self.frames = np.empty(self.shape, dtype='float32')
		self.exclude = np.zeros(self.shape, dtype='uint8')
		self.subtract = np.zeros(self.shape, dtype='float32')
		self.slots = []
		for k, case in enumerate(cases):
			t, j, i = k // (nrow * ncol), (k // ncol) % nrow, k % ncol
			v, ex, sub = case.cell()
			sl = (t, slice(j * box, (j + 1) * box), slice(i * box, (i + 1) * box))
			self.frames[sl], self.exclude[sl], self.subtract[sl] = v, ex, sub
			self.slots.append((t, j, i))

	def gather(self, per_cell):
		"""A ``(T, ny, nx)`` array of per-cell results in the order of ``cases``."""
		per_cell = np.asarray(per_cell)
		assert per_cell.shape == self.mesh_shape, (per_cell.shape, self.mesh_shape)
		return np.array([per_cell[s] for s in self.slots])


def mosaic(cases, box):
	return Mosaic(cases, box)


# ---------------------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
	return np.random.default_rng([20240, *key])


def _masked_rest(valid, npix, kinds=MASK_KINDS[:5]):
	"""``valid`` values, then masked pixels of every kind in ``kinds`` in turn, up to ``npix``: ``(values, exclude)``."""
	valid = np.asarray(valid, dtype='float32')
	k = np.arange(npix - valid.size) % len(kinds)
	rest = np.array([_MASK_VALUE[kinds[i]] for i in k], dtype='float32')
	excl = np.concatenate((np.zeros(valid.size, dtype=bool), np.array([kinds[i] == 'excluded' for i in k], dtype=bool)))
	return np.concatenate((valid, rest)), excl


def _truncated_normal(rng, level, sigma, size, cut=2.5):
	"""Gaussian noise without tails: nothing beyond ``cut`` sigma, so the clip stops once the outliers are gone."""
	z = rng.normal(0, 1, size)
	while np.any(np.abs(z) > cut):
		bad = np.abs(z) > cut
		z[bad] = rng.normal(0, 1, int(bad.sum()))
	return level + sigma * z


def _narrow(level, step, n_out, seed, npix=4096):
	"""``npix - n_out`` pixels on four neighbouring float32 steps at ``level``, ``n_out`` bright outliers."""
	rng = _rng(7, seed, n_out)
	core = F32(level) + rng.integers(0, 4, npix - n_out).astype('float32') * F32(step)
	assert np.all((core.astype('float64') - level) / step == np.round((core.astype('float64') - level) / step))    # the steps are representable
	return np.concatenate((core, rng.uniform(level + 50, 79000, n_out).astype('float32')))


#: (name, level, step, outliers, seeds): the first three lose the variance when the clipped keys are taken off running sums
NARROW_RECIPES = [
	('narrow_1000_2e-14', 1000.0, 2.0**-14, 96, (0, 1, 2)),
	('narrow_100_2e-17', 100.0, 2.0**-17, 400, (0, 1, 2)),
	('narrow_100_2e-12', 100.0, 2.0**-12, 400, (0, 1, 2)),
	('narrow_1000_2e-10', 1000.0, 2.0**-10, 96, (0,)),
	('narrow_100_1e-3', 100.0, 132 * 2.0**-17, 400, (0,)),     # (the first multiple of the float32 spacing at this level that is >= 1e-3)
]

#: tiers of outliers above a core uniform in 100 +- 1: (offset, count).  With tiers 1..k present, pass p removes exactly tier k + 1 - p
TIERS = [(10.0, 40), (60.0, 40), (400.0, 40), (3000.0, 40), (20000.0, 40)]


def _tiers(k, npix=4096):
	rng = _rng(3, k)
	n_out = sum(c for _, c in TIERS[:k])
	core = rng.uniform(99, 101, npix - n_out)
	return np.concatenate([core] + [100.0 + off + rng.uniform(0, 0.01 * off, c) for off, c in TIERS[:k]])


def cap_cell():
	"""Still clipping when the five passes are used up: the kept count differs between maxiters 4, 5 and 6."""
	return np.concatenate((_rng(4).normal(100, 1, 3000), 100 + np.geomspace(5, 60000, 1096)))


def bound_cell(outward):
	"""med = mean = 100 and std = 2 with every sum exact: 94 and 106 lie ON med +- 3 std and are kept; one float32 step further out
	(``outward``) all sixteen are clipped."""
	lo, hi = F32(94), F32(106)
	if outward:
		lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
	return np.concatenate((np.full(1976, 98.0), np.full(1976, 102.0), np.full(8, lo), np.full(8, hi), np.full(128, 100.0))).astype('float32')


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = {1: [100.0], 2: [100.0, 103.0], 3: [100.0, 101.0, 105.0], 4: [100.0, 101.0, 103.0, 110.0]}


def count_case(box, n, tag=''):
	npix = box * box
	valid = SMALL[n] if n in SMALL else _rng(1, box, n).normal(100, 3, n)
	v, _ = _masked_rest(valid, npix)
	return Case(f'count_{n}{tag}', box, v, n=n, **({'nmasked': npix, 'branch': 'nan'} if n == 0 else {}))


def sort_cases(box, n, tag):
	"""Six inputs that stress the sorting network, ``n`` valid pixels (the others NaN, spread through the cell)."""
	npix = box * box
	nan_at = np.round(np.linspace(5, npix - 3, npix - n)).astype(int) if n < npix else np.zeros(0, dtype=int)

	def with_nans(full):
		full = np.array(full, dtype='float32')
		full[nan_at] = np.nan
		return full
	e = np.arange(npix)
	pow2 = (n & (n - 1)) == 0          # integer keys and a power of two of them: every sum and the mean are exact
	out = [
		Case(f'sort_ascending{tag}', box, with_nans(50 + e / 64.0), scramble=False, n=n, passes=0, branch='mode'),
		Case(f'sort_descending{tag}', box, with_nans(50 + (npix - 1 - e) / 64.0), scramble=False, n=n, passes=0, branch='mode'),
		Case(f'sort_all_equal{tag}', box, with_nans(np.full(npix, 77.0)), n=n, passes=0, branch='mean', exact=True),
		Case(f'sort_alternating{tag}', box, with_nans(np.where(e % 2 == 0, 100.0, 104.0)), scramble=False, n=n, passes=0, exact=pow2),
		Case(f'sort_distinct{tag}', box, with_nans(10 + e / 32.0), n=n, passes=0, branch='mode'),
	]
	# keys of both signs through the subtract path: raw 0 .. 100, fifty taken off; raw -0.0 minus 0.0 is the key -0.0, raw 50 the key +0.0
	raw = (e % 101).astype('float32')
	sub = np.full(npix, 50.0, dtype='float32')
	zero = np.nonzero(raw == 0)[0][::2]
	raw[zero], sub[zero] = -0.0, 0.0
	out.append(Case(f'sort_mixed_sign{tag}', box, with_nans(raw), subtract=sub, n=n, passes=0, exact=pow2))
	return out


def box64_cases():
	B, N = 64, 4096
	cases = []
	# ---- counts
	for n in (0, 1, 2, 3, 4, 255, 256, 257, 4095, 4096):
		cases.append(count_case(B, n))
	for kind in MASK_KINDS:
		v, ex = _masked_rest([], N, kinds=(kind,))
		cases.append(Case(f'none_valid_{kind}', B, v, exclude=ex, n=0, nmasked=N, branch='nan'))
	v, ex = _masked_rest([], N, kinds=MASK_KINDS)
	cases.append(Case('none_valid_mixed', B, v, exclude=ex, n=0, nmasked=N, branch='nan'))
	# ---- the mask predicate: eight valid pixels far apart, so that one pixel more or less moves the mean by thousands and nothing is clipped
	tiny = np.nextafter(F32(0), F32(1))
	kept = [0.0, -0.0, tiny, F32(8e4), 2e4, 4e4, 6e4, 3e4]
	masked = [np.nextafter(F32(8e4), F32(np.inf)), F32(-1e-30), -tiny]
	v, _ = _masked_rest(kept + masked, N, kinds=('nan',))
	cases.append(Case('mask_predicate', B, v, n=8, nmasked=N - 8, passes=0))
	# ---- the sort
	cases += sort_cases(B, N, '_4096') + sort_cases(B, N - 7, '_4089')
	# ---- clip paths
	r = _rng(2)
	cases.append(Case('clip_none', B, r.uniform(90, 110, N), passes=0, sides=set()))
	cases.append(Case('clip_top', B, np.concatenate((r.uniform(98, 102, N - 96), r.uniform(200, 79000, 96))), sides={'top'}))
	cases.append(Case('clip_bottom', B, np.concatenate((_truncated_normal(r, 5000, 3, N - 96), r.uniform(0, 100, 96))), sides={'bottom'}))
	cases.append(Case('clip_both', B, np.concatenate((_truncated_normal(r, 1000, 5, N - 96), 1000 - r.uniform(500, 900, 48), 1000 + r.uniform(500, 900, 48))),
		passes=1, sides={'top', 'bottom'}))
	for k in (1, 2, 3, 4):
		cases.append(Case(f'clip_{k}_passes', B, _tiers(k), passes=k, sides={'top'}))
	cases.append(Case('clip_cap', B, cap_cell(), passes=5, cap=True))
	# ---- on the bound
	cases.append(Case('bound_on', B, bound_cell(False), exact=True, passes=0, nmasked=0, branch='mode'))
	cases.append(Case('bound_outside', B, bound_cell(True), passes=1, nmasked=16, sides={'top', 'bottom'}))
	# ---- estimator branches
	cases.append(Case('estimator_std_zero', B, np.concatenate((np.full(N - 96, 1000.0), r.integers(1050, 79000, 96))), exact=True, branch='mean', nmasked=96))
	cases.append(Case('estimator_mode', B, r.normal(100, 3, N), branch='mode'))
	cases.append(Case('estimator_median', B, np.where(r.random(N) < 0.6, 100.0, 110.0) + r.uniform(-0.5, 0.5, N), branch='median'))
	# ---- narrow cells with bright outliers
	for name, level, step, n_out, seeds in NARROW_RECIPES:
		for seed in seeds:
			cases.append(Case(f'{name}_seed{seed}', B, _narrow(level, step, n_out, seed), nmasked=n_out, sides={'top'}, narrow=True))
	return cases


def box16_cases():
	B, N = 16, 256
	r = _rng(16)
	return [count_case(B, 255), count_case(B, 256), count_case(B, 0), count_case(B, 1), count_case(B, 2), count_case(B, 129),
		Case('b16_outliers', B, np.concatenate((r.uniform(98, 102, N - 6), r.uniform(200, 79000, 6))), sides={'top'}, nmasked=6)] + sort_cases(B, N - 3, '_253')


def box50_cases():
	B, N = 50, 2500
	r = _rng(50)
	half = np.arange(N) % 2 == 1
	return [count_case(B, 2500), count_case(B, 2499), count_case(B, 0), count_case(B, 257),
		Case('b50_outliers', B, np.concatenate((r.uniform(98, 102, N - 60), r.uniform(200, 79000, 60))), sides={'top'}, nmasked=60),
		Case('b50_half_excluded', B, np.where(half, 300.0, 100.0) + r.uniform(-1, 1, N), exclude=half, n=1250, nmasked=1250, passes=0)] + sort_cases(B, N - 3, '_2497')


def box1_cases():
	tiny = np.nextafter(F32(0), F32(1))
	vals = [('valid', 5.0, 0), ('nan', np.nan, 1), ('negative', -1.0, 1), ('cutoff', F32(8e4), 0), ('above', np.nextafter(F32(8e4), F32(np.inf)), 1),
		('zero', 0.0, 0), ('inf', np.inf, 1), ('subnormal', tiny, 0), ('negative_subnormal', -tiny, 1), ('minus_zero', -0.0, 0)]
	return [Case(f'b1_{name}', 1, [v], exact=True, nmasked=nm, n=1 - nm, branch='nan' if nm else 'mean') for name, v, nm in vals]


def all_cases():
	"""``{box: [Case, ...]}``: one launch per box size."""
	return {64: box64_cases(), 16: box16_cases(), 50: box50_cases(), 1: box1_cases()}


# ---------------------------------------------------------------------------------------------------------------------------------
# frames that are no multiple of the box
# ---------------------------------------------------------------------------------------------------------------------------------
RAGGED_BOX = 64
RAGGED_SHAPE = (2, 64 + 33, 3 * 64 + 40)


def ragged_frames():
	"""
	``(frames, names)``: 2 x 4 cells of which the last row has 33 rows and the last column 40 columns inside the frame; the padded
	pixels are masked.  The values repeat 100 .. 103 (nothing is ever clipped), so ``nmasked`` is the padding plus the NaNs put
	in: in the last row 63, 64 and 65 of them bring cells (1, 0), (1, 1), (1, 2) to 2047, 2048 and 2049 masked pixels -- either side
	of the half that ``exclude_percentile = 50`` rejects from.  Frame 1 is frame 0 with other levels and the NaNs elsewhere.
	"""
	T, R, C = RAGGED_SHAPE
	yy, xx = np.mgrid[0:R, 0:C]
	f = np.stack([(100.0 + 50 * k + (3 * yy + 5 * xx + k) % 4) for k in range(T)]).astype('float32')
	for k in range(T):
		for i, n_nan in enumerate((63, 64, 65)):
			rows, cols = np.divmod(np.arange(n_nan) * (7 + 2 * k), 64)      # spread over the 33 x 64 pixels of the cell
			f[k, 64 + rows % 33, 64 * i + (cols + 11 * rows) % 64] = np.nan
	names = [f'ragged_{j}_{i}' for j in range(2) for i in range(4)]
	return f, names


def ragged_expected(f):
	"""Per frame ``(mesh, nmasked)`` of the oracle."""
	from oracle import backgrounds as ob
	return [ob.mesh_statistics(f[k], ob.stamp_mask(f[k], FLUX_CUTOFF), box=RAGGED_BOX) for k in range(f.shape[0])]


# ---------------------------------------------------------------------------------------------------------------------------------
# the clip, pass by pass, in the oracle's own statements (oracle.backgrounds.sigma_clip) -- for the host test
# ---------------------------------------------------------------------------------------------------------------------------------
def clip_trace(data, sigma=3.0, maxiters=5):
	"""
	``oracle.backgrounds.sigma_clip`` statement by statement, recording every pass that looked at the data: ``m`` samples, ``med``,
	``std``, the number clipped ``below`` / ``above``, and ``margin`` = the smallest distance of a sample from a clip bound in units
	of ``std`` (inf where ``std == 0`` and no sample differs from the median).  Returns ``(kept data, [pass, ...])``.
	"""
	data = np.asarray(data, dtype='float64')
	trace = []
	for _ in range(maxiters):
		if data.size == 0:
			break
		med = np.median(data)
		std = np.std(data)
		lo, hi = med - sigma*std, med + sigma*std
		keep = (data >= lo) & (data <= hi)
		dist = np.minimum(np.abs(data - lo), np.abs(data - hi)).min()
		trace.append({'m': data.size, 'med': med, 'std': std, 'below': int(np.sum(data < lo)), 'above': int(np.sum(data > hi)),
			'margin': (dist / std) if std > 0 else (np.inf if dist > 0 or np.all(data == med) else 0.0), 'data': data})
		if np.all(keep):
			break
		data = data[keep]
	return data, trace
