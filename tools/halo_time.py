#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of Halo photometry's TV-min optimiser (csrc/halo.hip, ``tp_halo_tvmin``) on the two sizes of DESIGN.md ("Halo"): 64 FFI
problems of 484 pixels x 1 300 cadences and one 2-min-cadence problem of 1 257 pixels x 19 000 cadences.  Reports the wall time
per call, the evaluations (forward passes) and accepted points (backward passes) from the context's kernel profile, the P bytes
read (one pass per forward and per backward) and their share of the 8 TB/s HBM peak, and the CPU restatement's time on one host
core (``--cpu``).  Writes a JSON line to ``--out``.
"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes / s


def problem(npix, ncad, seed):
	rng = np.random.default_rng(seed)
	base = rng.uniform(50, 1000, npix)
	walk = np.cumsum(rng.normal(size=ncad)) * 0.01
	P = base[None, :] * (1 + 1e-3 * np.sin(np.arange(ncad) / 7.0))[:, None] * (1 + 0.05 * walk[:, None] * rng.normal(size=npix)[None, :])
	P = (P + rng.normal(size=(ncad, npix)) * 2).astype('float32')
	return P, rng.random(ncad) >= 0.05


def measure(ctx, name, probs, repeat, cpu):
	from photometry_amd import halo
	halo.tvmin(ctx, probs)   # warm-up: allocation cache, code objects
	walls = []
	for _ in range(repeat):
		ctx.sync()
		t0 = time.perf_counter()
		r = halo.tvmin(ctx, probs)
		walls.append(time.perf_counter() - t0)
	# one more call with the kernel profile on (events around every launch: not part of the wall times above)
	ctx.profile(True)
	ctx.profile_reset()
	halo.tvmin(ctx, probs)
	prof = ctx.profile_report()
	ctx.profile(False)
	repeat = 1
	# host-side packing and copies are part of tvmin's wall time; the device time is the sum of the halo kernels
	kern = {k: {'n': n, 'ms': ms} for k, (n, ms) in prof.items() if k.startswith('tp_halo_')}
	dev_ms = sum(v['ms'] for v in kern.values()) / repeat
	pbytes = sum(4 * p[0].shape[0] * ((p[0].shape[1] + 3) // 4 * 4) for p in probs)
	n_fwd = kern.get('tp_halo_forward_kernel', {}).get('n', 0) / repeat
	n_bwd = kern.get('tp_halo_backward_kernel', {}).get('n', 0) / repeat
	res = {'case': name, 'problems': len(probs), 'wall_ms': 1e3 * min(walls), 'device_ms': dev_ms,
		'kernel_ms': {k: v['ms'] / repeat for k, v in kern.items()}, 'launches': {k: v['n'] / repeat for k, v in kern.items()},
		'iterations': {int(i): int(n) for i, n in zip(*np.unique(r['iterations'], return_counts=True))},
		'status': {int(s): int(n) for s, n in zip(*np.unique(r['status'], return_counts=True))},
		'P_bytes': pbytes}
	# every step launches the forward pass over all active problems: bytes of P read per evaluation x evaluations of the slowest
	# problem is a lower bound on the bytes moved; the share of peak below uses the forward + backward kernel times
	fb_ms = sum(kern.get(k, {}).get('ms', 0.0) for k in ('tp_halo_forward_kernel', 'tp_halo_backward_kernel')) / repeat
	res['forward_launches'] = n_fwd
	res['backward_launches'] = n_bwd
	res['P_passes_upper'] = n_fwd + n_bwd
	res['share_of_hbm_peak_fwd_bwd'] = (n_fwd + n_bwd) * pbytes / (fb_ms * 1e-3) / HBM_PEAK if fb_ms else None
	res['share_of_hbm_peak_wall'] = (n_fwd + n_bwd) * pbytes / min(walls) / HBM_PEAK
	if cpu:
		import halo_common as hc
		t0 = time.perf_counter()
		for P, fit in probs:
			hc.lbfgs(P, fit)
		res['cpu_restatement_s'] = time.perf_counter() - t0
	print(json.dumps(res))
	return res


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--repeat', type=int, default=3)
	ap.add_argument('--cpu', action='store_true', help='also time the CPU restatement (one host core)')
	ap.add_argument('--out', default=None)
	a = ap.parse_args()
	from photometry_amd.device import Context
	ffi = [problem(484, 1300, seed=i) for i in range(64)]
	big = [problem(1257, 19000, seed=100)]
	with Context(0) as ctx:
		out = [measure(ctx, '64 x 484 px x 1300 cad', ffi, a.repeat, a.cpu), measure(ctx, '1 x 1257 px x 19000 cad', big, a.repeat, a.cpu)]
	if a.out:
		with open(a.out, 'a') as fh:
			for r in out:
				fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
	main()
