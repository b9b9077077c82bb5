#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of the image movement kernels (csrc/motion.hip) on a sector-sized stack resident in HBM: ``--frames`` frames of
``--size`` x ``--size`` (default 1 300 of 2048 x 2048), built on the device from ``--distinct`` star fields rendered at
sub-pixel shifts.  Reports ms per frame for tp_motion_prepare and tp_motion_ecc (translation), the iteration histogram and the
bytes per iteration the design must move (blurred frame + template, 8 B per pixel), and writes a JSON line to ``--out``.

Kernel times come from a separate ``rocprofv3 --kernel-trace --stats -- python tools/motion_time.py ...`` run.
"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes / s


def star_field(R, C, shift, stars, sigma=1.0, background=100.0):
	"""pixel-integrated Gaussian stars (each in a 15 x 15 window) at ``shift`` = (column, row)."""
	from scipy.special import erf
	rows, cols, flux = stars
	img = np.full((R, C), background)
	d = np.sqrt(2) * sigma
	for r, c, f in zip(rows + shift[1], cols + shift[0], flux):
		r0, c0 = int(r) - 7, int(c) - 7
		rr = np.arange(r0, r0 + 15)
		cc = np.arange(c0, c0 + 15)
		gr = 0.5 * (erf((rr - r + 0.5) / d) - erf((rr - r - 0.5) / d))
		gc = 0.5 * (erf((cc - c + 0.5) / d) - erf((cc - c - 0.5) / d))
		img[r0:r0 + 15, c0:c0 + 15] += f * np.outer(gr, gc)
	return img.astype('float32')


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--frames', type=int, default=1300)
	ap.add_argument('--size', type=int, default=2048)
	ap.add_argument('--distinct', type=int, default=24)
	ap.add_argument('--stars', type=int, default=4000)
	ap.add_argument('--chunk-mib', type=int, default=0, help='blurred frames per chunk, MiB (0: the library default)')
	ap.add_argument('--repeat', type=int, default=2)
	ap.add_argument('--out', default=None)
	a = ap.parse_args()
	from photometry_amd import motion
	from photometry_amd.device import Context
	R = C = a.size
	rng = np.random.default_rng(1)
	stars = (rng.uniform(10, R - 10, a.stars), rng.uniform(10, C - 10, a.stars), 10 ** rng.uniform(2.5, 5.0, a.stars))
	shifts = np.vstack([[0.0, 0.0], rng.uniform(-0.5, 0.5, (a.distinct - 1, 2))])
	base = np.stack([star_field(R, C, s, stars) for s in shifts])
	base += rng.normal(0, 2.0, base.shape).astype('float32')
	res = {'frames': a.frames, 'size': a.size, 'distinct': a.distinct}
	with Context(0) as ctx:
		d_base = ctx.array(base)
		stack = ctx.empty((a.frames, R, C), 'float32')
		fb = R * C * 4
		for k in range(a.frames):
			ctx._check(ctx.lib.tp_memcpy_d2d(ctx.handle, stack.ptr + k * fb, d_base.ptr + (k % a.distinct) * fb, fb))
		ctx.sync()
		for rep in range(a.repeat):
			t0 = time.perf_counter()
			prepared = motion.prepare_frames(ctx, stack)
			ctx.sync()
			t1 = time.perf_counter()
			r = motion.ecc_prepared(ctx, prepared.slice0(0, 1), prepared, 'translation', chunk_bytes=a.chunk_mib << 20)
			ctx.sync()
			t2 = time.perf_counter()
			prepared.free()
			print(f"run {rep}: prepare {1e3 * (t1 - t0) / a.frames:.3f} ms/frame, ecc {1e3 * (t2 - t1) / a.frames:.3f} ms/frame, "
				f"sector {t2 - t0:.3f} s")
		err = np.abs(r['kernels'] - shifts[np.arange(a.frames) % a.distinct]).max()
		hist = np.bincount(r['iterations'])
		iters = int(r['iterations'].sum())
		res.update({'prepare_ms_per_frame': 1e3 * (t1 - t0) / a.frames, 'ecc_ms_per_frame': 1e3 * (t2 - t1) / a.frames,
			'sector_s': t2 - t0, 'iteration_histogram': {int(i): int(n) for i, n in enumerate(hist) if n},
			'frame_iterations': iters, 'bytes_per_frame_iteration': 8 * R * C, 'max_error_px': float(err),
			'status': {int(s): int(n) for s, n in zip(*np.unique(r['status'], return_counts=True))}})
		# the iteration kernel's share of HBM peak at the wall time of the whole ECC (an upper bound on its time)
		res['ecc_bytes'] = iters * 8 * R * C
		res['ecc_share_of_hbm_peak_wall'] = res['ecc_bytes'] / (t2 - t1) / HBM_PEAK
	print(json.dumps(res))
	if a.out:
		with open(a.out, 'a') as fh:
			fh.write(json.dumps(res) + '\n')


if __name__ == '__main__':
	main()
