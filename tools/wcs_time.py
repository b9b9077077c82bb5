#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of the 'wcs' movement kernel (csrc/wcs.hip): LinPSF positions (tp_wcs_star_positions) of ``--rows`` catalogue rows in
stamps of ``--batch`` rows over ``--cadences`` cadences, each cadence its own TAN-SIP frame (order-4 SIP, CRVAL / CD drifting by
arcseconds).  Reports the median wall time of the call (synchronised), the kernel time from the context's profile, the bytes
the positions write (2 x 8 B per row and cadence) and that as a fraction of HBM peak; then ``jitter`` of one point over the
series (the pos_corr call).  Writes a JSON line to ``--out``.
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


def header(rng, dra=0.0, ddec=0.0, rot=0.0):
	s = 21.0 / 3600
	c, n = np.cos(np.deg2rad(rot)), np.sin(np.deg2rad(rot))
	cd = s * np.array([[-c, n], [n, c]])
	cards = {'CTYPE1': 'RA---TAN-SIP', 'CTYPE2': 'DEC--TAN-SIP', 'CRPIX1': 1045.0, 'CRPIX2': 1001.0, 'CRVAL1': 84.1 + dra,
		'CRVAL2': -62.3 + ddec, 'CD1_1': cd[0, 0], 'CD1_2': cd[0, 1], 'CD2_1': cd[1, 0], 'CD2_2': cd[1, 1], 'A_ORDER': 4, 'B_ORDER': 4}
	r = np.random.default_rng(7)
	for p in range(5):
		for q in range(5 - p):
			if p + q >= 2:
				cards[f'A_{p}_{q}'] = r.normal(0, 2.0) / 1000.0 ** (p + q)
				cards[f'B_{p}_{q}'] = r.normal(0, 2.0) / 1000.0 ** (p + q)
	return cards


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--rows', type=int, default=300000)
	ap.add_argument('--batch', type=int, default=30)
	ap.add_argument('--cadences', type=int, default=1300)
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--out', default=None)
	a = ap.parse_args()
	from photometry_amd import wcs as W
	from photometry_amd.device import Context
	from photometry_amd.motion import MovementKernel
	ctx = Context(0)
	rng = np.random.default_rng(1)
	T = a.cadences
	hdrs = [header(rng, 2.0 / 3600 * np.sin(k / 50.0), 1.5 / 3600 * np.cos(k / 40.0), 3.0 / 3600 * np.sin(k / 30.0)) for k in range(T)]
	ref = W.TanSipWCS.from_header(hdrs[0])
	d_params = ctx.array(W.pack([W.TanSipWCS.from_header(h) for h in hdrs]))
	n = a.rows
	xy32 = np.column_stack((rng.uniform(0, 2100, n), rng.uniform(0, 2050, n))).astype('float32')
	base = (xy32 - np.float32(1000.0)).astype('float32')
	offsets = np.arange(0, n + a.batch, a.batch).clip(max=n).astype('int64')
	offsets = np.unique(offsets)
	k1 = np.arange(T, dtype='int32')
	k2 = np.full(T, -1, dtype='int32')
	zeros = np.zeros(T)
	out_index = np.arange(n, dtype='int64')
	walls = []
	ctx.profile(True)
	for rep in range(a.reps + 1):
		if rep == 1:
			ctx.profile_reset()
		ctx.sync()
		t0 = time.perf_counter()
		pc, pr, st = W.star_positions(ctx, d_params, T, ref, offsets, xy32, base[:, 0], base[:, 1], out_index, n, k1, k2, zeros, zeros)
		ctx.sync()
		if rep:
			walls.append(time.perf_counter() - t0)
		del pc, pr
	prof = ctx.profile_report()
	kern = {k: v for k, v in prof.items() if 'wcs' in k}
	npos, mspos = kern.get('tp_wcs_positions_kernel', (0, float('nan')))
	kms = mspos / max(npos, 1)
	nbytes = 2.0 * 8 * n * T
	mk = MovementKernel('wcs', wcs_ref=hdrs[0], ctx=ctx)
	mk.load_series(np.arange(T, dtype='float64'), hdrs)
	tj = []
	for rep in range(a.reps + 1):
		t0 = time.perf_counter()
		mk.jitter(np.arange(T, dtype='float64') + 0.25, 812.3, 640.7)
		if rep:
			tj.append(time.perf_counter() - t0)
	res = {'rows': n, 'batch': a.batch, 'cadences': T, 'positions_wall_ms': 1e3 * float(np.median(walls)), 'positions_kernel_ms': kms,
		'bytes_written': nbytes, 'hbm_fraction_kernel': nbytes / (kms * 1e-3) / HBM_PEAK if kms == kms else None,
		'status_nonzero_rows': int(np.count_nonzero(st)), 'jitter_one_point_ms': 1e3 * float(np.median(tj)), 'profile': kern}
	print(json.dumps(res))
	if a.out:
		with open(a.out, 'a') as f:
			f.write(json.dumps(res) + '\n')
	ctx.close()


if __name__ == '__main__':
	main()
