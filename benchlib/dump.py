# -*- coding: utf-8 -*-
"""
``bench.py --dump-outputs DIR``: what the timed path computed in its last step, as ``DIR/<name>.npy``, so that two builds can
be compared output for output (with the same arguments the inputs are the same seeded scene).

The arrays are those ``sharded.ShardedRun.collect`` hands a caller: ``lc`` ``(5, N, T)`` (flux, flux_err, flux_background,
centroid column / row), ``contamination``, ``status``, ``flags``, ``mask`` and, with the LinPSF fit, ``psf_flux``,
``psf_contamination``, ``psf_status``.  Integers become float64 (float32 for one- and two-byte types such as the mask): exact
for every value they hold.

Every file holds finite numbers only.  The step's floating-point outputs carry NaN by the reference's own rules (the flux of a
cadence with a NaN pixel in the mask, AperturePhotometry's ``np.sum``), so each of them is written as two files without losing
anything: ``<name>.npy`` with every non-finite entry set to 0, and ``<name>_nonfinite.npy`` (float32, same shape) with the code
of every entry -- 0 finite, 1 NaN, 2 +inf, 3 -inf.

When the whole set would exceed ``MAX_BYTES``, every array keeps the same fixed, seeded sample of targets; ``target_index.npy``
lists the targets written, in the order they appear.
"""
import os
import numpy as np

MAX_BYTES = 64 * 10**6
SAMPLE_SEED = 20261015
_HEADER_BYTES = 4096   # an upper bound of the .npy header of one file
NONFINITE_SUFFIX = '_nonfinite'


def target_axis(name):
	return 1 if name == 'lc' else 0


def as_float(a):
	a = np.asarray(a)
	if a.dtype in (np.float32, np.float64):
		return a
	return a.astype('float32' if a.dtype.itemsize <= 2 else 'float64')


def split_nonfinite(a):
	"""``(values, code)``: ``a`` with every non-finite entry 0, and the float32 code of every entry (0 finite, 1 NaN, 2 +inf, 3 -inf)."""
	code = np.zeros(a.shape, dtype='float32')
	code[np.isnan(a)] = 1
	code[np.isposinf(a)] = 2
	code[np.isneginf(a)] = 3
	return np.where(code == 0, a, np.zeros((), dtype=a.dtype)), code


def sample_targets(n_targets, bytes_per_target, budget):
	"""Sorted indices of the targets written: all of them when they fit in ``budget`` bytes, else a fixed, seeded sample."""
	k = min(n_targets, budget // bytes_per_target)
	if k < 1:
		raise ValueError(f'the outputs of one target ({bytes_per_target} bytes) exceed the dump budget of {budget} bytes')
	if k == n_targets:
		return np.arange(n_targets)
	return np.sort(np.random.default_rng(SAMPLE_SEED).choice(n_targets, size=k, replace=False))


def dump_outputs(outputs, dirname, n_targets, max_bytes=MAX_BYTES):
	"""Writes ``outputs`` (``{name: array}``, the target axis of length ``n_targets``) under ``dirname``; returns the target indices."""
	floating = {name for name, a in outputs.items() if np.asarray(a).dtype.kind == 'f'}   # the ones that get a _nonfinite file
	arrays = {name: as_float(a) for name, a in outputs.items()}
	for name, a in arrays.items():
		if a.shape[target_axis(name)] != n_targets:
			raise ValueError(f'{name}: shape {a.shape} has no target axis of length {n_targets}')
	bytes_per_target = 8 + sum((a.nbytes + (a.size * 4 if name in floating else 0)) // n_targets for name, a in arrays.items())
	n_files = len(arrays) + len(floating) + 1                                       # + target_index (8 bytes per target above)
	idx = sample_targets(n_targets, bytes_per_target, max_bytes - _HEADER_BYTES * n_files)
	os.makedirs(dirname, exist_ok=True)
	for name, a in arrays.items():
		if len(idx) < n_targets:
			a = np.take(a, idx, axis=target_axis(name))
		if name in floating:
			a, code = split_nonfinite(a)
			np.save(os.path.join(dirname, name + NONFINITE_SUFFIX + '.npy'), code)
		np.save(os.path.join(dirname, name + '.npy'), np.ascontiguousarray(a))
	np.save(os.path.join(dirname, 'target_index.npy'), idx.astype('float64'))
	return idx
