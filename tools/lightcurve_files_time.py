#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of the light-curve files of the batched frames entry (``BatchResults.save_lightcurves``, photometry_amd/lcfile.py; the
``QUALITY`` column from ``tp_stamp_flag_series``, csrc/stampflags.hip) on a synthetic region: ``--targets`` (2 500)
targets x ``--cadences`` (1 300) on ``--size`` x ``--size`` (512) pixels with a pixel-flag stack whose BackgroundShenanigans bit is set
at density 1e-4.  Nothing is asserted; one JSON line per step, appended to ``--out``.  After one warm-up pass every step is run
three times; all three times are given beside the best.

``flags``    ``tp_stamp_flag_series`` over the batch's final stamps: the kernel from device timers (``tp_profile_get``), the call with
             its upload and its download of ``(N, T)`` int32 from a host clock, and the numpy restatement of the same reduction
             (``np.any(flags[:, r1:r2, c1:c2] & 4, axis=(1, 2))`` per target) on one host core;
``files``    ``save_lightcurves`` at ``workers`` 1 and 16 and ``compresslevel`` 9 and 1: files per second, and the share of the
             workers' time spent in gzip (the rest builds the bytes of the HDUs); ``--compress device`` and, with it, ``--table host
             device``: the device's DEFLATE encoder and the ``LIGHTCURVE`` data units written on the device (``tp_lc_table_pack``);
``plugin``   the per-target plugin loop (``run_plugin(AperturePhotometry, ...)`` with its ``save_lightcurve``) over the first
             ``--plugin-targets`` targets: what a caller had to do for the files before.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_region(np, N, T, FR, seed=7):
	"""Frames ``(T, FR, FR)``, flags, catalogue and targets: stars of Tmag 8 .. 14 on a flat sky, one shared noise pool of 8 frames."""
	rng = np.random.default_rng(seed)
	rows, cols = rng.uniform(12, FR - 12, N), rng.uniform(12, FR - 12, N)
	tmag = rng.uniform(8.0, 14.0, N)
	img = np.zeros((FR, FR))
	yy, xx = np.mgrid[-4:5, -4:5]
	for r, c, m in zip(rows, cols, tmag):
		ri, ci = int(round(r)), int(round(c))
		img[ri - 4:ri + 5, ci - 4:ci + 5] += 10**(-0.4 * (m - 20.451)) * np.exp(-0.5 * ((yy + ri - r)**2 + (xx + ci - c)**2) / 0.81) / (2 * np.pi * 0.81)
	noise = np.sqrt(np.abs(img) + 200.0).astype('float32')
	pool = rng.standard_normal((8, FR, FR)).astype('float32') * noise
	gain = (1 + 1e-3 * rng.normal(size=T)).astype('float32')
	images = np.empty((T, FR, FR), dtype='float32')
	for t in range(T):
		images[t] = img.astype('float32') * gain[t] + 30.0 + pool[t % 8]
	frames = {'images': images, 'images_err': np.broadcast_to(noise, (T, FR, FR)), 'backgrounds': np.broadcast_to(np.float32(100.0), (T, FR, FR))}
	flags = rng.integers(0, 4, (T, FR, FR), dtype='uint8')
	flags[rng.random((T, FR, FR), dtype='float32') < 1e-4] |= 4
	cat = {'starid': np.arange(N, dtype='int64') + 1, 'tmag': tmag.astype('float32'), 'row': rows.astype('float32'), 'column': (cols + 44).astype('float32')}
	targets = {'starid': cat['starid'].copy(), 'tmag': tmag, 'row': rows, 'column': cols + 44}
	return frames, flags, cat, targets


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--targets', type=int, default=2500)
	ap.add_argument('--cadences', type=int, default=1300)
	ap.add_argument('--size', type=int, default=512)
	ap.add_argument('--repeats', type=int, default=3)
	ap.add_argument('--plugin-targets', type=int, default=32)
	ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory, removed afterwards)')
	ap.add_argument('--out', default=None)
	ap.add_argument('--compress', choices=('zlib', 'device'), nargs='+', default=['zlib'], help="how the files are compressed; 'device': one run per worker count")
	ap.add_argument('--compresslevel', type=int, nargs='+', default=[9, 1], help="gzip's levels with --compress zlib")
	ap.add_argument('--table', choices=('host', 'device'), nargs='+', default=['host'], help="who writes the LIGHTCURVE data units; 'device' runs with --compress device only")
	ap.add_argument('--skip-baselines', action='store_true', help='the files alone: no flag-series timing on the host, no per-target plugin')
	a = ap.parse_args()
	import numpy as np
	from photometry_amd import pipeline, tessphot_frames
	from photometry_amd.device import Context
	from photometry_amd.lcfile import FileInfo, save_lightcurves, PIXEL_BACKGROUND_SHENANIGANS, CORRECTOR_BACKGROUND_SHENANIGANS
	from photometry_amd.plugins import AperturePhotometry
	from photometry_amd.source import MemoryStampSource
	from photometry_amd.tessphot import run_plugin

	def emit(res):
		print(json.dumps(res), flush=True)
		if a.out:
			with open(a.out, 'a') as fh:
				fh.write(json.dumps(res) + '\n')

	N, T, FR = a.targets, a.cadences, a.size
	frames, flags, cat, targets = make_region(np, N, T, FR)
	tstamp = 1500.0 + np.arange(T) * 1800.0 / 86400.0
	quality = np.zeros(T, dtype='int32')
	with tempfile.TemporaryDirectory(dir=a.dir) as root, Context(0) as ctx:
		stack = pipeline.FrameStack(ctx, dict(frames, pixel_flags=flags), 0, 44)
		t0 = time.perf_counter()
		res = tessphot_frames(ctx, stack, targets, cat, tstamp, quality)
		res = tessphot_frames(ctx, stack, targets, cat, tstamp, quality)      # (the second call: stacks transposed, code objects loaded)
		ctx.sync()
		emit({'step': 'photometry', 'targets': N, 'cadences': T, 'two_calls_s': time.perf_counter() - t0, 'with_file': int(((res.status == 1) | (res.status == 3)).sum())})
		wanted = (res.status == 1) | (res.status == 3)
		stamps = np.where(wanted[:, None], np.asarray(res.stamp, dtype='int64'), -1)

		# ---- the flag series ----
		stack.stamp_flag_series(stamps, PIXEL_BACKGROUND_SHENANIGANS, CORRECTOR_BACKGROUND_SHENANIGANS)
		ctx.profile(True)
		kernel_ms, call_ms = [], []
		for _ in range(a.repeats):
			ctx.profile_reset()
			t0 = time.perf_counter()
			series = stack.stamp_flag_series(stamps, PIXEL_BACKGROUND_SHENANIGANS, CORRECTOR_BACKGROUND_SHENANIGANS)
			call_ms.append((time.perf_counter() - t0) * 1e3)
			kernel_ms.append(ctx.profile_report()['tp_stamp_flags_kernel'][1])
		ctx.profile(False)
		host_ms = []
		for _ in range(0 if a.skip_baselines else a.repeats):
			t0 = time.perf_counter()
			ref = np.zeros((N, T), dtype='int32')
			for i, (r1, r2, c1, c2) in enumerate(stamps):
				if r1 >= 0:
					ref[i, np.any(flags[:, r1:r2, c1 - 44:c2 - 44] & 4, axis=(1, 2))] = CORRECTOR_BACKGROUND_SHENANIGANS
			host_ms.append((time.perf_counter() - t0) * 1e3)
		if not a.skip_baselines:
			emit({'step': 'flags', 'targets': N, 'cadences': T, 'stack_MB': flags.nbytes / 1e6, 'kernel_ms': kernel_ms, 'kernel_ms_best': min(kernel_ms), 'call_ms': call_ms,
				'call_ms_best': min(call_ms), 'numpy_one_core_ms': host_ms, 'numpy_one_core_ms_best': min(host_ms), 'equal': bool(np.array_equal(series, ref)),
				'flagged_pairs': int((series != 0).sum())})

		# ---- the files ----
		info = FileInfo(14, 2, 3)
		for table in (a.table if a.compress[-1] == 'device' else ['host']):      # warm-up
			save_lightcurves(res, stack, os.path.join(root, 'warm'), info, tstamp, quality, 6, targets=targets, workers=16, compresslevel=1, compress=a.compress[-1], table=table)
		n_files = int(wanted.sum())
		for compress, table, workers, level in [(c, t, w, l) for c in a.compress for t in (a.table if c == 'device' else ['host'])
				for l in (a.compresslevel if c == 'zlib' else a.compresslevel[:1]) for w in (1, 16)]:
			runs = []
			for k in range(a.repeats):
				timings = {}
				t0 = time.perf_counter()
				paths = save_lightcurves(res, stack, os.path.join(root, f'w{workers}l{level}'), info, tstamp, quality, 6, targets=targets, workers=workers,
					compresslevel=level, timings=timings, compress=compress, table=table)
				runs.append({'wall_s': time.perf_counter() - t0, 'quality_s': timings['quality'], 'build_s': timings['build'], 'table_s': timings.get('table'), 'place_s': timings.get('place'),
					'gzip_s': timings['gzip'], 'write_s': timings.get('write'), 'gzip_parts_s': timings.get('gzip_parts')})
			best = min(runs, key=lambda r: r['wall_s'])
			size = sum(os.path.getsize(p) for p in paths if p is not None)
			deflate_kernels = None
			if compress == 'device':                                          # once more under the kernel profile
				ctx.profile(True)
				ctx.profile_reset()
				save_lightcurves(res, stack, os.path.join(root, f'w{workers}l{level}'), info, tstamp, quality, 6, targets=targets, workers=workers, compress='device', table=table)
				ctx.sync()
				deflate_kernels = {k: v for k, v in ctx.profile_report().items() if 'deflate' in k or 'tp_lc_' in k}
				ctx.profile(False)
			emit({'step': 'files', 'workers': workers, 'compress': compress, 'table': table, 'deflate_kernels': deflate_kernels, 'compresslevel': level if compress == 'zlib' else None, 'files': n_files, 'runs': runs, 'files_per_s': n_files / best['wall_s'],
				'gzip_share_of_worker_time': best['gzip_s'] / (best['gzip_s'] + best['build_s']), 'quality_share_of_wall': best['quality_s'] / best['wall_s'],
				'MB_written': size / 1e6})

		if a.skip_baselines:
			return
		# ---- the per-target plugin ----
		src = MemoryStampSource({k: np.moveaxis(v, 0, 2) for k, v in dict(frames, pixel_flags=flags).items()}, 0, 44, tstamp, np.zeros(T), np.arange(T), quality, cat,
			targets=targets, sector=14, camera=2, ccd=3)
		m = min(a.plugin_targets, N)
		run_plugin(AperturePhotometry, int(targets['starid'][0]), src, os.path.join(root, 'plugin'), ctx=ctx)
		runs = []
		for _ in range(a.repeats):
			t0 = time.perf_counter()
			wrote = 0
			for i in range(m):
				p = run_plugin(AperturePhotometry, int(targets['starid'][i]), src, os.path.join(root, 'plugin'), ctx=ctx)
				wrote += 'filepath_lightcurve' in p._details
			runs.append(time.perf_counter() - t0)
		emit({'step': 'plugin', 'targets': m, 'files': wrote, 'runs_s': runs, 'targets_per_s': m / min(runs), 'ms_per_target': min(runs) / m * 1e3})


if __name__ == '__main__':
	main()
