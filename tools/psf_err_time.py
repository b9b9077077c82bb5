#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of the PSFPhotometry flux-error pass (csrc/psf_err.hip, ``tp_psf_flux_err``) beside the fit it leaves untouched,
on the batch of ``tools/psf_time.py``: 4 096 targets x 50 cadences x 15 x 15, up to five fitted stars per target
(``simulate.make_scene(seed=7)``), SPOC grid.

Two steps, each a process of its own under its own time limit (``--limit`` seconds), the second only if the first ended well:
``fit``      ``engine.psf_fit`` alone: wall time per call and ``tp_psf_fit_kernel`` from ``tp_profile_get``;
``fit_err``  the same call followed by ``engine.psf_flux_err`` on the fit's own ``params``: the same kernel plus ``tp_psf_err_kernel``,
             the pass's time and its share of the fit's.
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


def run_step(step, n_targets, n_cad, n_steps):
	import numpy as np
	from photometry_amd import simulate, engine, psf as hpsf
	from photometry_amd.device import Context, DeviceCube
	from photometry_amd.plugins import psf_star_selection, mag2flux
	Nt, T, H, W = n_targets, n_cad, 15, 15
	with Context(0) as ctx:
		s = simulate.make_scene(Nt, T, H, W, seed=7)
		simulate.fill_cubes(s, nan_fraction=0.001)
		prf = simulate.synthetic_prf(seed=1)
		model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
		offs, params, mini = [0], [], []
		for i in range(Nt):
			c = s.catalog_of(i)
			sel = psf_star_selection(c['row_stamp'], c['column_stamp'], c['tmag'], s.target_pos_row[i] - s.stamps[i][0], s.target_pos_column[i] - s.stamps[i][2], s.target_tmag[i])
			params.append(np.column_stack((c['row_stamp'][sel].astype('float64'), c['column_stamp'][sel].astype('float64'), mag2flux(c['tmag'][sel].astype('float64')))))
			offs.append(offs[-1] + len(sel))
			m = np.zeros((H, W), dtype='uint8')
			r, cc = int(round(s.target_pos_row[i] - s.stamps[i][0])), int(round(s.target_pos_column[i] - s.stamps[i][2]))
			m[max(r - 1, 0):r + 2, max(cc - 1, 0):cc + 2] = 1
			mini.append(m)
		coef = engine.linpsf_prf(ctx, ctx.array(model.base_coef), ctx.array(model.weights(s.stamps)))
		images, backgrounds = DeviceCube.from_host(ctx, s.images), DeviceCube.from_host(ctx, s.backgrounds)
		tx, ty, d_offs, d_mini = ctx.array(model.tx), ctx.array(model.ty), ctx.array(np.asarray(offs, dtype='int64')), ctx.array(np.stack(mini))
		d_params0 = ctx.array(np.concatenate(params))
		err_cube = DeviceCube.from_host(ctx, s.images_err) if step == 'fit_err' else None
		ferr = ctx.zeros((Nt, T), 'float64') if step == 'fit_err' else None
		last = {}

		def one():
			last['fit'] = engine.psf_fit(ctx, images, backgrounds, coef, tx, ty, d_offs, d_params0, d_mini)
			if step == 'fit_err':
				engine.psf_flux_err(ctx, images, backgrounds, err_cube, coef, tx, ty, d_offs, last['fit']['params'], d_mini, out=ferr)
		one()
		ctx.sync()
		ctx.profile(True)
		ctx.profile_reset()
		walls = []
		for _ in range(n_steps):
			t0 = time.perf_counter()
			one()
			ctx.sync()
			walls.append((time.perf_counter() - t0) * 1e3)
		ctx.profile(False)
		kern = {k: {'launches': c, 'ms_per_step': t / n_steps} for k, (c, t) in ctx.profile_report().items() if k.startswith('tp_psf')}
		nit = last['fit']['nit'].to_host()
		counts = np.diff(np.asarray(offs))
		res = {'step': step, 'targets': Nt, 'cadences': T, 'stamp': [H, W], 'fitted_stars': int(offs[-1]),
			'targets_by_star_count': {str(k): int(np.sum(np.minimum(counts, 5) == k)) for k in range(6)}, 'steps': n_steps,
			'wall_ms_per_step': walls, 'kernels': kern, 'simplex_iterations': int(nit.sum())}
		if step == 'fit_err':
			host, flux = ferr.to_host(), last['fit']['flux'].to_host()
			ms, fit_ms = kern['tp_psf_err_kernel']['ms_per_step'], kern['tp_psf_fit_kernel']['ms_per_step']
			res.update({'err_kernel_ms': ms, 'fit_wall_ms': float(np.mean(walls)) - ms, 'share_of_fit_kernel_time': ms / fit_ms,
				'flux_err_finite_fraction': float(np.mean(np.isfinite(host))), 'flux_finite_fraction': float(np.mean(np.isfinite(flux))),
				'nan_pattern_equal_to_flux': bool(np.array_equal(np.isnan(host), np.isnan(flux))), 'flux_err_median': float(np.nanmedian(host))})
		print(json.dumps(res))
		return res


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--step', choices=('fit', 'fit_err'), default=None, help='run one step in this process (default: both, each a child process)')
	ap.add_argument('--targets', type=int, default=4096)
	ap.add_argument('--cadences', type=int, default=50)
	ap.add_argument('--steps', type=int, default=3)
	ap.add_argument('--limit', type=int, default=240, help='time limit of a step, seconds')
	ap.add_argument('--out', default=None)
	a = ap.parse_args()
	if a.step is not None:
		res = run_step(a.step, a.targets, a.cadences, a.steps)
		if a.out:
			with open(a.out, 'a') as fh:
				fh.write(json.dumps(res) + '\n')
		return 0
	for step in ('fit', 'fit_err'):
		cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--targets', str(a.targets), '--cadences', str(a.cadences), '--steps', str(a.steps)]
		cmd += ['--out', a.out] if a.out else []
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
