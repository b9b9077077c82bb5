#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of Halo photometry over a batch of target pixel files (``photometry_amd.tessphot_tpfs(method='halo')``) beside the
per-file loop it stands for, on synthetic files of a bright star at 2-minute cadence: ``--height`` x ``--width`` pixels (default 21 x 21;
the largest Halo problem is 1 257 pixels), ``--rows`` cadences (default 19 000), every second file with a gap of one day in the middle
(two segments).  The files sit in the page cache.  Nothing is asserted; one JSON line per step, appended to ``--out``.

Steps, all in one process, each timed with a host clock around work that ends with its results on the host, after one warm-up pass:
``batch``         ``tessphot_tpfs(method='halo')`` without files written, every result built (``results[i]``): files/s;
``batch_files``   the same with ``output_folder``: the light-curve files with their ``WEIGHTMAP`` written;
``profile``       one more ``batch`` under the per-kernel profile: the milliseconds of every kernel and the shares of select (stat, cad,
                  compact), gather, solver (``tp_halo_tvmin``'s kernels) and outputs (norm, lightcurve) among the Halo kernels;
``plugin``        per file ``load_tpfs([file])``, ``TpfStampSource`` and ``HaloPhotometry.photometry()``: the problems built in numpy from
                  a host copy of the cube;
``plugin_files``  per file ``tessphot('halo', starid, TpfStampSource(...), folder, datasource='tpf')``, which writes the light curve.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_files(root, n, H, W, rows):
	"""n TPFs of a ``Tmag = 5`` star that fills its stamp (a wide PSF: light on every edge) over a noisy background, each file its own
	place on the CCD, its own ``TICID`` and its own brightness; every second one has a gap of a day in the middle.  Returns ``(files,
	catalog)``."""
	import numpy as np
	from photometry_amd import fitsio
	rng = np.random.default_rng(1)
	yy, xx = np.mgrid[0:H, 0:W]
	cy, cx = (H - 1) / 2 + 0.2, (W - 1) / 2 - 0.1
	sigma2 = (0.3 * min(H, W))**2
	star = 10**(-0.4 * (5.0 - 20.451)) * np.exp(-0.5 * ((yy - cy)**2 + (xx - cx)**2) / sigma2) / (2 * np.pi * sigma2)
	# the star's light varies by 0.1 %, every pixel's share of it drifts slowly (what the weights are there to cancel)
	drift = 1 + 2e-3 * np.sin(2 * np.pi * np.arange(rows) / 700.0)[:, None, None] * ((xx - cx) / W)[None]
	flux = (star[None] * drift * (1 + 1e-3 * rng.normal(size=rows))[:, None, None] + rng.normal(0.0, 12.0, size=(rows, H, W))).astype('float32')
	err = np.sqrt(np.abs(flux) + 200.0).astype('float32')
	bkg = np.full((rows, H, W), 100.0, dtype='float32')
	quality = np.zeros(rows, dtype='int32')
	quality[rng.random(rows) < 0.02] = 32
	image = lambda name, fmt, array: {'name': name, 'format': f'{H * W}{fmt}', 'array': array, 'dim': (W, H)} # noqa: E731
	files, cat = [], {'starid': [], 'tmag': [], 'row': [], 'column': []}
	for k in range(n):
		c1p, c2p = 100 + 60 * (k % 30), 100 + 60 * (k // 30)
		t = 1683.35 + 1e-4 * k + np.arange(rows) * (120.0 / 86400.0)
		if k % 2:
			t[rows // 2:] += 1.0
		cols = [{'name': 'TIME', 'format': 'D', 'array': t}, {'name': 'TIMECORR', 'format': 'E', 'array': np.full(rows, 3e-3, dtype='float32')},
			{'name': 'CADENCENO', 'format': 'J', 'array': np.arange(rows, dtype='int32')}, image('RAW_CNTS', 'J', flux.astype('int32')), image('FLUX', 'E', flux * np.float32(1 + 0.01 * k)),
			image('FLUX_ERR', 'E', err), image('FLUX_BKG', 'E', bkg), image('FLUX_BKG_ERR', 'E', bkg * np.float32(0.01)),
			{'name': 'QUALITY', 'format': 'J', 'array': quality}, {'name': 'POS_CORR1', 'format': 'E', 'array': np.zeros(rows, dtype='float32')},
			{'name': 'POS_CORR2', 'format': 'E', 'array': np.zeros(rows, dtype='float32')}]
		path = os.path.join(root, 'tess2019199201929-s0014-%016d-0150-s_tp.fits' % (1000 + k))
		fitsio.write(path, [fitsio.primary_hdu([fitsio.card('TELESCOP', 'TESS'), fitsio.card('SECTOR', 14), fitsio.card('CAMERA', 1), fitsio.card('CCD', 1), fitsio.card('DATA_REL', 35),
				fitsio.card('TICID', 1000 + k)]),
			fitsio.bintable_hdu('PIXELS', cols, [fitsio.card('TIMEDEL', 120.0 / 86400.0)]),
			fitsio.image_hdu('APERTURE', np.ones((H, W), dtype='int32'), [fitsio.card('CRVAL1P', c1p), fitsio.card('CRVAL2P', c2p)])])
		files.append(path)
		cat['starid'].append(1000 + k)
		cat['tmag'].append(5.0)
		cat['row'].append(c2p - 1 + cy)
		cat['column'].append(c1p - 1 + cx)
	catalog = {'starid': np.array(cat['starid'], dtype='int64'), 'tmag': np.array(cat['tmag'], dtype='float32'), 'row': np.array(cat['row'], dtype='float32'),
		'column': np.array(cat['column'], dtype='float32')}
	return files, catalog


#: the Halo kernels of the profile by the step they belong to
STEPS = {'select': ('tp_halo_cube_stat_kernel', 'tp_halo_cube_cad_kernel', 'tp_halo_cube_compact_kernel'), 'gather': ('tp_halo_cube_gather_kernel',),
	'solver': ('tp_halo_init_kernel', 'tp_halo_forward_kernel', 'tp_halo_stat_kernel', 'tp_halo_backward_kernel', 'tp_halo_finish_kernel', 'tp_halo_output_kernel'),
	'outputs': ('tp_halo_cube_norm_kernel', 'tp_halo_cube_lightcurve_kernel')}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--files', type=int, default=4, help='synthetic TPFs (168 MB each at the default shape; few enough for the page cache)')
	ap.add_argument('--height', type=int, default=21)
	ap.add_argument('--width', type=int, default=21)
	ap.add_argument('--rows', type=int, default=19000)
	ap.add_argument('--plugin-files', type=int, default=None, help='files of the per-file baselines (default: all)')
	ap.add_argument('--repeats', type=int, default=3)
	ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory, removed afterwards)')
	ap.add_argument('--out', default=None)
	ap.add_argument('--skip-baselines', action='store_true', help='stop behind the batched entry: no per-file runs')
	a = ap.parse_args()
	from photometry_amd import tpf, tessphot, tessphot_tpfs, STATUS
	from photometry_amd.device import Context
	from photometry_amd.plugins import HaloPhotometry

	def emit(res):
		print(json.dumps(res), flush=True)
		if a.out:
			with open(a.out, 'a') as fh:
				fh.write(json.dumps(res) + '\n')

	with tempfile.TemporaryDirectory(dir=a.dir) as root, Context(0) as ctx:
		ini = os.path.join(root, 'settings.ini')
		with open(ini, 'w') as fh:
			fh.write('[halo]\nenabled = true\n')
		os.environ['TESSPHOT_SETTINGS'] = ini
		files, catalog = make_files(root, a.files, a.height, a.width, a.rows)
		N = len(files)
		out_dir = os.path.join(root, 'lc')
		for ld in tpf.load_tpfs(ctx, files):                                  # warm-up: page cache, code objects, the allocation cache
			ld.free()

		def best_of(fn, repeats=a.repeats):
			times, last = [], None
			for _ in range(repeats):
				t0 = time.perf_counter()
				last = fn()
				times.append(time.perf_counter() - t0)
			return min(times), times, last

		shape = {'height': a.height, 'width': a.width, 'rows': a.rows, 'file_bytes': sum(os.path.getsize(f) for f in files)}

		# ---- the batched entry ----
		def batch(folder=None):
			status, segments, iterations = [], [], []
			for res in tessphot_tpfs(ctx, files, catalog, output_folder=folder, version=6 if folder else None, method='halo'):
				for i in range(len(res)):
					r = res[i]
					status.append(r.status)
					segments.append(0 if r.halo_weightmap is None else len(r.halo_weightmap['weightmap']))
				iterations += [int(v) for part in res.halo.parts for it in part.iterations for v in it]
			return status, segments, iterations
		batch()                                                               # warm-up
		t, times, (status, segments, iterations) = best_of(batch)
		emit(dict(shape, step='batch', files=N, ok_or_warning=sum(s in (STATUS.OK, STATUS.WARNING) for s in status), segments=segments, iterations=iterations,
			files_per_s=N / t, ms_per_file=t / N * 1e3, all_s=times))

		def batch_files():
			shutil.rmtree(out_dir, ignore_errors=True)
			return batch(out_dir)
		batch_files()
		t, times, _ = best_of(batch_files)
		emit(dict(shape, step='batch_files', files=N, written=len(os.listdir(out_dir)), files_per_s=N / t, ms_per_file=t / N * 1e3, all_s=times))

		ctx.profile(True)
		ctx.profile_reset()
		t0 = time.perf_counter()
		batch()
		ctx.sync()
		wall = time.perf_counter() - t0
		report = ctx.profile_report()
		ctx.profile(False)
		halo_ms = {step: sum(report.get(k, (0, 0.0))[1] for k in names) for step, names in STEPS.items()}
		total = sum(halo_ms.values()) or 1.0
		emit(dict(shape, step='profile', files=N, wall_s=wall, kernels={k: {'launches': n, 'ms': ms} for k, (n, ms) in sorted(report.items())},
			halo_ms=halo_ms, halo_share={k: v / total for k, v in halo_ms.items()}, all_kernels_ms=sum(ms for _, ms in report.values())))
		if a.skip_baselines:
			return 0

		# ---- the per-file baselines ----
		some = files[:a.plugin_files] if a.plugin_files else files
		ids = [1000 + k for k in range(len(some))]

		def plugin():
			status = []
			for path, starid in zip(some, ids):
				(ld,) = tpf.load_tpfs(ctx, [path])
				with HaloPhotometry(starid, tpf.TpfStampSource(ld, catalog), None, datasource='tpf', ctx=ctx) as pho:
					pho.photometry()
					status.append(pho.status)
				ld.free()
			return status
		plugin()                                                              # warm-up
		t, times, status = best_of(plugin, max(1, a.repeats - 1))
		emit(dict(shape, step='plugin', files=len(some), ok_or_warning=sum(s in (STATUS.OK, STATUS.WARNING) for s in status), files_per_s=len(some) / t,
			ms_per_file=t / len(some) * 1e3, all_s=times))

		def plugin_files():
			shutil.rmtree(out_dir, ignore_errors=True)
			status = []
			for path, starid in zip(some, ids):
				(ld,) = tpf.load_tpfs(ctx, [path])
				pho = tessphot('halo', starid, tpf.TpfStampSource(ld, catalog), out_dir, datasource='tpf', ctx=ctx, version=6)
				status.append(pho.status)
				ld.free()
			return status
		t, times, status = best_of(plugin_files, max(1, a.repeats - 1))
		emit(dict(shape, step='plugin_files', files=len(some), written=len(os.listdir(out_dir)), files_per_s=len(some) / t, ms_per_file=t / len(some) * 1e3, all_s=times))
	return 0


if __name__ == '__main__':
	sys.exit(main())
