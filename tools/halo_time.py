#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of Halo photometry's TV-min optimiser (csrc/halo.hip, ``tp_halo_tvmin``) on the two sizes of DESIGN.md ("Halo"): 64 FFI
problems of 484 pixels x 1 300 cadences and one 2-min-cadence problem of 1 257 pixels x 19 000 cadences.  Reports the wall time
per call, the evaluations (forward passes) and accepted points (backward passes) from the context's kernel profile, the P bytes
read (one pass per forward and per backward) and their share of the 8 TB/s HBM peak, and the CPU restatement's time on one host
core (``--cpu``).  Writes a JSON line to ``--out``.

``--frames``: the batched entry instead -- 32 bright targets (64 two-segment problems of a 23 x 23 Halo stamp x 1 300 cadences) on a
resident frame stack: wall and per-kernel device time of (a) ``pipeline.halo_frames`` (problems built, packed and normalised on the
device) and (b) the per-target way (the cube cut on the host, ``halo.photometry``: numpy packs P and it is uploaded), same process,
same data, and their ratio.
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


def frames_scene(n_side=(4, 8), T=1300, pitch=26, seed=5):
	"""A region of ``n_side`` bright stars on a grid (one Halo stamp each, none clipped), float32 ``(T, R, C)`` stacks."""
	rng = np.random.default_rng(seed)
	R, C = pitch * n_side[0] + 4, pitch * n_side[1] + 4
	rows = (np.arange(n_side[0]) * pitch + pitch // 2 + 2.3)[:, None] + np.zeros(n_side[1])[None, :]
	cols = np.zeros(n_side[0])[:, None] + (np.arange(n_side[1]) * pitch + pitch // 2 + 2.6)[None, :]
	rows, cols = rows.ravel() + 100, cols.ravel() + 200
	yy, xx = np.mgrid[0:R, 0:C]
	img = np.full((R, C), 50.0)
	for r, c in zip(rows, cols):
		img += 3e5 * np.exp(-0.5 * ((yy + 100 - r)**2 + (xx + 200 - c)**2) / 9.0)
	walk = np.cumsum(rng.normal(size=T)) * 1e-4
	images = (img[None] * (1 + walk)[:, None, None] + rng.normal(size=(T, R, C)) * 5).astype('float32')
	frames = {'images': images, 'images_err': np.sqrt(np.abs(images) + 100).astype('float32'), 'backgrounds': np.full((T, R, C), 50.0, dtype='float32')}
	n = len(rows)
	targets = {'starid': np.arange(n, dtype='int64') + 1, 'tmag': np.full(n, 5.5), 'row': rows, 'column': cols}
	time_ = 1354.0 + np.arange(T) * 1800.0 / 86400.0      # sector 2: 27 days round the split at 1368.0
	quality = np.where(rng.random(T) < 0.05, 32, 0).astype('int32')
	return frames, 100, 200, time_, quality, targets


def halo_kernels(prof):
	return {k: {'n': n, 'ms': ms} for k, (n, ms) in prof.items() if k.startswith('tp_halo_')}


def measure_frames(ctx, repeat):
	from photometry_amd import halo, pipeline
	from photometry_amd.plugins import load_settings, mag2flux
	frames, row0, col0, time_, quality, targets = frames_scene()
	T, n = len(time_), len(targets['starid'])
	settings = load_settings()
	settings.set('halo', 'enabled', 'true')
	stack = pipeline.FrameStack(ctx, frames, row0, col0)
	cat = {k: targets[k] for k in ('starid', 'tmag', 'row', 'column')}

	def batched():
		return pipeline.halo_frames(ctx, stack, targets, cat, time_, quality, sector=2, settings=settings)

	first = batched()
	hwt = {k: np.moveaxis(frames[k], 0, 2) for k in ('images', 'images_err')}

	def per_target():
		out = []
		for i in range(n):
			st = first.stamp[i]
			cut = [np.ascontiguousarray(hwt[k][st[0] - row0:st[1] - row0, st[2] - col0:st[3] - col0]) for k in ('images', 'images_err')]
			out.append(halo.photometry(ctx, cut[0], cut[1], quality, time_, np.zeros(T), np.arange(T), first.pixel_mask[i], 2, mag2flux(targets['tmag'][i])))
		return out

	ref = per_target()
	same = all(np.array_equal(first.flux[i], ref[i]['flux'], equal_nan=True) for i in range(n))
	res = {'case': f'frames: {n} targets, {n * first.f.shape[1]} problems of {int(first.pixel_mask[0].sum())} px x {T} cad', 'flux_bit_equal': bool(same)}
	for name, fn in (('halo_frames', batched), ('per_target', per_target)):
		walls = []
		for _ in range(repeat):
			ctx.sync()
			t0 = time.perf_counter()
			fn()
			walls.append(time.perf_counter() - t0)
		ctx.profile(True)
		ctx.profile_reset()
		fn()
		kern = halo_kernels(ctx.profile_report())
		ctx.profile(False)
		dev = sum(v['ms'] for v in kern.values())
		build = sum(v['ms'] for k, v in kern.items() if any(w in k for w in ('select', 'gather', 'norm', 'lightcurve')))
		res[name] = {'wall_ms': 1e3 * min(walls), 'device_ms': dev, 'wall_minus_device_ms': 1e3 * min(walls) - dev, 'build_and_output_kernels_ms': build,
			'optimiser_kernels_ms': dev - build, 'kernel_ms': {k: v['ms'] for k, v in kern.items()}, 'launches': {k: v['n'] for k, v in kern.items()}}
	res['wall_ratio_per_target_over_frames'] = res['per_target']['wall_ms'] / res['halo_frames']['wall_ms']
	print(json.dumps(res))
	return res


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--repeat', type=int, default=3)
	ap.add_argument('--frames', action='store_true', help='time the batched frames entry against the per-target path instead')
	ap.add_argument('--cpu', action='store_true', help='also time the CPU restatement (one host core)')
	ap.add_argument('--out', default=None)
	a = ap.parse_args()
	from photometry_amd.device import Context
	with Context(0) as ctx:
		if a.frames:
			out = [measure_frames(ctx, a.repeat)]
		else:
			ffi = [problem(484, 1300, seed=i) for i in range(64)]
			big = [problem(1257, 19000, seed=100)]
			out = [measure(ctx, '64 x 484 px x 1300 cad', ffi, a.repeat, a.cpu), measure(ctx, '1 x 1257 px x 19000 cad', big, a.repeat, a.cpu)]
	if a.out:
		with open(a.out, 'a') as fh:
			for r in out:
				fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
	main()
