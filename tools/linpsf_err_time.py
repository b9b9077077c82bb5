#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of the LinPSF flux-error pass (csrc/linpsf_err.hip, ``tp_linpsf_flux_err``) beside the fit it leaves
untouched, on the benchmark's LinPSF batch: 10 000 targets x 1 300 cadences x 15 x 15, up to three fitted stars per target
(``simulate.make_scene(seed=1000)``), SPOC grid, raw cube resident with the background series subtracted on the fly.

Two steps, each a process of its own under its own time limit (``--limit`` seconds), the second only if the first ended well:
``fit``      ``pipeline.linpsf_step`` alone: the kernel times from ``tp_profile_get`` per step;
``fit_err``  the same step followed by ``engine.linpsf_flux_err``: the same kernels plus ``tp_linpsf_err_kernel``, and the share of
             the FP64 vector peak the error pass reaches (its algorithmic flops: per star, cadence and pixel inside the cut-off the
             13 x 13 contraction, 13 x (4 + 13) multiply-adds; per cadence and finite pixel S (S + 1) multiply-adds for G and W).
Prints one JSON line per step and appends them to ``--out``.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VALU_PEAK = 78.6e12   # MI355X, FP64 vector flop/s


def run_step(step, n_targets, n_steps):
	import numpy as np
	from photometry_amd import simulate, engine, pipeline, psf as hpsf
	from photometry_amd.device import Context
	Nt, T, H, W = n_targets, 1300, 15, 15
	with Context(0) as ctx:
		scene = simulate.make_scene(Nt, T, H, W, seed=1000)
		scene.aperture = None
		cubes = engine.synth_fill(ctx, scene, images=False, images_err=(step == 'fit_err'), backgrounds=False, raw=True)
		bkg_raw = engine.background_stamp(ctx, cubes['raw'])
		bkg = engine.smooth_time(ctx, bkg_raw, T, 3)
		prf = simulate.synthetic_prf(seed=1)
		model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
		batch = pipeline.LinPSFBatch(ctx, scene, model, images=cubes['raw'], subtract=bkg)
		ferr = ctx.zeros((Nt, T), 'float64') if step == 'fit_err' else None

		def one():
			pipeline.linpsf_step(ctx, batch)
			if step == 'fit_err':
				engine.linpsf_flux_err(ctx, batch.images, cubes['images_err'], batch.coef, batch.tx, batch.ty, batch.star_offsets, batch.target_index,
					batch.pos_row, batch.pos_col, batch.max_stars, out=ferr)
		one()
		ctx.sync()
		ctx.profile(True)
		ctx.profile_reset()
		t0 = time.perf_counter()
		for _ in range(n_steps):
			one()
		ctx.sync()
		wall = (time.perf_counter() - t0) / n_steps * 1e3
		ctx.profile(False)
		kern = {k: {'launches': c, 'ms_per_step': t / n_steps} for k, (c, t) in ctx.profile_report().items() if k.startswith('tp_linpsf')}
		res = {'step': step, 'targets': Nt, 'cadences': T, 'stamp': [H, W], 'fitted_stars': int(batch.n_fit_stars), 'max_stars': int(batch.max_stars),
			'steps': n_steps, 'wall_ms_per_step': wall, 'kernels': kern}
		if step == 'fit_err':
			counts = np.diff(batch.star_offsets_h)
			fma = batch.n_fit_stars * T * 79.0 * 13 * 17 + float(np.sum(counts * (counts + 1))) * T * H * W
			ms = kern['tp_linpsf_err_kernel']['ms_per_step']
			host = ferr.to_host()
			res.update({'err_kernel_ms': ms, 'algorithmic_flops': 2 * fma, 'fraction_of_fp64_vector_peak': 2 * fma / (ms * 1e-3) / FP64_VALU_PEAK,
				'flux_err_finite_fraction': float(np.mean(np.isfinite(host))), 'flux_err_median': float(np.nanmedian(host))})
		print(json.dumps(res))
		return res


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--step', choices=('fit', 'fit_err'), default=None, help='run one step in this process (default: both, each a child process)')
	ap.add_argument('--targets', type=int, default=10000)
	ap.add_argument('--steps', type=int, default=3)
	ap.add_argument('--limit', type=int, default=240, help='time limit of a step, seconds')
	ap.add_argument('--out', default=None)
	a = ap.parse_args()
	if a.step is not None:
		res = run_step(a.step, a.targets, a.steps)
		if a.out:
			with open(a.out, 'a') as fh:
				fh.write(json.dumps(res) + '\n')
		return 0
	for step in ('fit', 'fit_err'):
		cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--targets', str(a.targets), '--steps', str(a.steps)] + (['--out', a.out] if a.out else [])
		try:
			rc = subprocess.run(cmd, timeout=a.limit).returncode
		except subprocess.TimeoutExpired:
			print(f'{step}: no result within {a.limit} s', file=sys.stderr)
			return 124
		if rc != 0:   # nothing more on the device after a failure
			print(f'{step}: exit status {rc}', file=sys.stderr)
			return rc
	return 0


if __name__ == '__main__':
	sys.exit(main())
