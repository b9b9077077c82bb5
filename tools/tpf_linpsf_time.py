#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of LinPSF photometry over a batch of target pixel files (``photometry_amd.tessphot_tpfs(method='linpsf')``) beside
the per-file loop it stands for, on synthetic two-minute-shaped files: ``--height`` x ``--width`` pixels (default 11 x 11), ``--rows``
cadences (default 19 000), a target with two fitted neighbours, ``POS_CORR1/2`` of a few hundredths of a pixel, a synthetic PRF
(``simulate.synthetic_prf``).  The files sit in the page cache.  Nothing is asserted; one JSON line per step, appended to ``--out``.

Steps, all in one process, each timed with a host clock around work that ends with its results on the host, after one warm-up pass:
``load``           ``tpf.load_tpf_groups`` alone (and the cubes freed): what every batched step below begins with;
``batch``          ``tessphot_tpfs(method='linpsf')`` with ``[linpsf] flux_errors`` off, no files, every result built (``results[i]``);
``batch_err``      the same with the flux errors on;
``batch_err_files``  the same with ``output_folder``: the light-curve files written (none is written with the errors off);
``profile``        one more ``batch_err`` under the per-kernel profile: the milliseconds of the positions kernel, the PRF blend, the fit,
                   the error pass, the diagnostics and the sum image (the loader's kernels run on its own context and are in ``load``);
``plugin`` / ``plugin_err``  per file ``load_tpfs([file])``, ``TpfStampSource(..., prf=model)`` and ``LinPSFPhotometry.photometry()`` with the
                   errors off / on, on the first ``--plugin-files`` files;
``plugin_err_files``  per file ``tessphot('linpsf', ...)`` with the errors on, which writes the light curve.
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
	"""n TPFs of a ``Tmag = 9.5`` star with two neighbours inside five pixels, each file its own place on the CCD, its own ``TICID`` and its
	own ``POS_CORR``.  Returns ``(files, starid, catalog)``."""
	import numpy as np
	from photometry_amd import fitsio
	rng = np.random.default_rng(1)
	yy, xx = np.mgrid[0:H, 0:W]
	stars = [(9.5, (H - 1) / 2 + 0.2, (W - 1) / 2 - 0.1), (11.0, (H - 1) / 2 + 2.4, (W - 1) / 2 + 1.3), (12.0, (H - 1) / 2 - 1.9, (W - 1) / 2 - 2.2)]
	img = np.zeros((H, W))
	for tm, r, c in stars:
		img += 10**(-0.4 * (tm - 20.44)) * np.exp(-0.5 * ((yy - r)**2 + (xx - c)**2) / 0.81) / (2 * np.pi * 0.81)
	flux = (img[None] * (1 + 1e-3 * rng.normal(size=rows))[:, None, None] + rng.normal(0.0, 12.0, size=(rows, H, W))).astype('float32')
	err = np.sqrt(np.abs(flux) + 200.0).astype('float32')
	bkg = np.full((rows, H, W), 100.0, dtype='float32')
	quality = np.zeros(rows, dtype='int32')
	quality[rng.random(rows) < 0.02] = 32
	image = lambda name, fmt, array: {'name': name, 'format': f'{H * W}{fmt}', 'array': array, 'dim': (W, H)} # noqa: E731
	files, starid, cat = [], [], {'starid': [], 'tmag': [], 'row': [], 'column': []}
	for k in range(n):
		c1p, c2p = 100 + 40 * (k % 40), 100 + 40 * (k // 40)
		t = 1683.35 + 1e-4 * k + np.arange(rows) * (120.0 / 86400.0)
		cols = [{'name': 'TIME', 'format': 'D', 'array': t}, {'name': 'TIMECORR', 'format': 'E', 'array': np.full(rows, 3e-3, dtype='float32')},
			{'name': 'CADENCENO', 'format': 'J', 'array': np.arange(rows, dtype='int32')}, image('RAW_CNTS', 'J', flux.astype('int32')), image('FLUX', 'E', flux * np.float32(1 + 0.01 * k)),
			image('FLUX_ERR', 'E', err), image('FLUX_BKG', 'E', bkg), image('FLUX_BKG_ERR', 'E', bkg * np.float32(0.01)),
			{'name': 'QUALITY', 'format': 'J', 'array': quality}, {'name': 'POS_CORR1', 'format': 'E', 'array': (rng.normal(size=rows) * 0.03).astype('float32')},
			{'name': 'POS_CORR2', 'format': 'E', 'array': (rng.normal(size=rows) * 0.03).astype('float32')}]
		path = os.path.join(root, 'tess2019199201929-s0014-%016d-0150-s_tp.fits' % (1000 + k))
		fitsio.write(path, [fitsio.primary_hdu([fitsio.card('TELESCOP', 'TESS'), fitsio.card('SECTOR', 14), fitsio.card('CAMERA', 1), fitsio.card('CCD', 1), fitsio.card('DATA_REL', 35),
				fitsio.card('TICID', 1000 + k)]),
			fitsio.bintable_hdu('PIXELS', cols, [fitsio.card('TIMEDEL', 120.0 / 86400.0)]),
			fitsio.image_hdu('APERTURE', np.ones((H, W), dtype='int32'), [fitsio.card('CRVAL1P', c1p), fitsio.card('CRVAL2P', c2p)])])
		files.append(path)
		starid.append(1000 + k)
		for j, (tm, r, c) in enumerate(stars):
			cat['starid'].append(1000 + k if j == 0 else 100000 * j + k)
			cat['tmag'].append(tm)
			cat['row'].append(c2p - 1 + r)
			cat['column'].append(c1p - 1 + c)
	catalog = {'starid': np.array(cat['starid'], dtype='int64'), 'tmag': np.array(cat['tmag'], dtype='float32'), 'row': np.array(cat['row'], dtype='float32'),
		'column': np.array(cat['column'], dtype='float32')}
	return files, starid, catalog


#: the kernels of the profile by the step they belong to
STEPS = {'positions': ('tp_star_positions_targets_kernel',), 'prf': ('tp_linpsf_prf_kernel',),
	'fit': ('tp_linpsf_plan_kernel', 'tp_linpsf_coef_kernel', 'tp_linpsf_fit_kernel', 'tp_linpsf_fit_direct_kernel', 'tp_linpsf_fitm_kernel', 'tp_linpsf_finalize_kernel'),
	'error_pass': ('tp_linpsf_err_kernel',), 'diagnostics': ('tp_diagnostics_kernel',), 'sumimage': ('tp_sumimage_kernel',)}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--files', type=int, default=12, help='synthetic TPFs (46 MB each at the default shape; few enough for the page cache)')
	ap.add_argument('--height', type=int, default=11)
	ap.add_argument('--width', type=int, default=11)
	ap.add_argument('--rows', type=int, default=19000)
	ap.add_argument('--plugin-files', type=int, default=None, help='files of the per-file baselines (default: all)')
	ap.add_argument('--repeats', type=int, default=3)
	ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory, removed afterwards)')
	ap.add_argument('--out', default=None)
	ap.add_argument('--skip-baselines', action='store_true', help='stop behind the batched entry: no per-file runs')
	a = ap.parse_args()
	from photometry_amd import tpf, tessphot, tessphot_tpfs, simulate, STATUS, psf as hpsf
	from photometry_amd.device import Context
	from photometry_amd.plugins import LinPSFPhotometry

	def emit(res):
		print(json.dumps(res), flush=True)
		if a.out:
			with open(a.out, 'a') as fh:
				fh.write(json.dumps(res) + '\n')

	with tempfile.TemporaryDirectory(dir=a.dir) as root, Context(0) as ctx:
		ini = os.path.join(root, 'settings.ini')
		with open(ini, 'w') as fh:
			fh.write('[linpsf]\nflux_errors = true\n')

		def errors(on):
			if on:
				os.environ['TESSPHOT_SETTINGS'] = ini
			else:
				os.environ.pop('TESSPHOT_SETTINGS', None)
		files, starid, catalog = make_files(root, a.files, a.height, a.width, a.rows)
		prf = simulate.synthetic_prf(seed=2)
		model = hpsf.PRFModel(prf['values'], prf['ccdColumn'], prf['ccdRow'], prf['prfColumn'], prf['prfRow'])
		N = len(files)
		out_dir = os.path.join(root, 'lc')

		def best_of(fn, repeats=a.repeats):
			times, last = [], None
			for _ in range(repeats):
				t0 = time.perf_counter()
				last = fn()
				times.append(time.perf_counter() - t0)
			return min(times), times, last

		shape = {'height': a.height, 'width': a.width, 'rows': a.rows, 'file_bytes': sum(os.path.getsize(f) for f in files)}

		def load():
			groups, _ = tpf.load_tpf_groups(ctx, files)
			ctx.sync()
			for g in groups:
				g.free()
		load()                                                                # warm-up: page cache, code objects, the allocation cache
		t, times, _ = best_of(load)
		emit(dict(shape, step='load', files=N, files_per_s=N / t, ms_per_file=t / N * 1e3, all_s=times))

		# ---- the batched entry ----
		def batch(folder=None):
			status, finite = [], 0
			for res in tessphot_tpfs(ctx, files, catalog, output_folder=folder, version=6 if folder else None, method='linpsf', prf=model):
				for i in range(len(res)):
					r = res[i]
					status.append(r.status)
					finite += int((r.lightcurve['flux'] == r.lightcurve['flux']).sum())
			return status, finite
		for step, on, folder in (('batch', False, None), ('batch_err', True, None), ('batch_err_files', True, out_dir)):
			errors(on)

			def run():
				shutil.rmtree(out_dir, ignore_errors=True)
				return batch(folder)
			run()                                                             # warm-up
			t, times, (status, finite) = best_of(run)
			emit(dict(shape, step=step, files=N, ok_or_warning=sum(s in (STATUS.OK, STATUS.WARNING) for s in status), finite_flux=finite,
				written=len(os.listdir(out_dir)) if folder and os.path.isdir(out_dir) else 0, files_per_s=N / t, ms_per_file=t / N * 1e3, all_s=times))

		errors(True)
		ctx.profile(True)
		ctx.profile_reset()
		t0 = time.perf_counter()
		batch()
		ctx.sync()
		wall = time.perf_counter() - t0
		report = ctx.profile_report()
		ctx.profile(False)
		step_ms = {step: sum(report.get(k, (0, 0.0))[1] for k in names) for step, names in STEPS.items()}
		emit(dict(shape, step='profile', files=N, wall_s=wall, kernels={k: {'launches': n, 'ms': ms} for k, (n, ms) in sorted(report.items())},
			step_ms=step_ms, all_kernels_ms=sum(ms for _, ms in report.values())))
		if a.skip_baselines:
			return 0

		# ---- the per-file baselines ----
		some = files[:a.plugin_files] if a.plugin_files else files
		ids = starid[:len(some)]

		def plugin(folder=None):
			status = []
			for path, sid in zip(some, ids):
				(ld,) = tpf.load_tpfs(ctx, [path])
				src = tpf.TpfStampSource(ld, catalog, prf=model)
				if folder is None:
					# (no file: the plugin's photometry alone; with the errors off it ends in the reference's ValueError)
					with LinPSFPhotometry(sid, src, None, datasource='tpf', ctx=ctx) as pho:
						try:
							pho.photometry()
						except ValueError:
							pho._status = STATUS.ERROR
				else:
					pho = tessphot('linpsf', sid, src, folder, datasource='tpf', ctx=ctx, version=6)
				status.append(pho.status)
				ld.free()
			return status
		for step, on, folder in (('plugin', False, None), ('plugin_err', True, None), ('plugin_err_files', True, out_dir)):
			errors(on)

			def run():
				shutil.rmtree(out_dir, ignore_errors=True)
				return plugin(folder)
			if step == 'plugin':
				run()                                                         # warm-up
			t, times, status = best_of(run, max(1, a.repeats - 1))
			emit(dict(shape, step=step, files=len(some), ok_or_warning=sum(s in (STATUS.OK, STATUS.WARNING) for s in status),
				written=len(os.listdir(out_dir)) if folder and os.path.isdir(out_dir) else 0, files_per_s=len(some) / t, ms_per_file=t / len(some) * 1e3, all_s=times))
	return 0


if __name__ == '__main__':
	sys.exit(main())
