#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of a batched run over target pixel files (``photometry_amd.tessphot_tpfs``) on synthetic files of the shape of a
2-minute target (11 x 11 pixels, 19 000 rows, 46.5 MB) that sit in the page cache, beside the per-file plugin loop it replaces.
Nothing is asserted; one JSON line per step, appended to ``--out``.

Steps, all in one process, each timed with a host clock around work that ends with its results on the host, after one warm-up pass:
``load``          ``tpf.load_tpfs`` over all files (the reader's ceiling: cubes of one target each);
``groups``        ``tpf.load_tpf_groups`` over all files (the same stream into cubes of many targets);
``batch``         ``tessphot_tpfs`` without files written, every result built (``results[i]``): files/s;
``batch_files``   the same with ``output_folder``: the light-curve files written (gzip level 9 on the worker pool), and the seconds the
                  workers spent building and compressing;
``plugin``        the baseline without files: per file ``load_tpfs([file])``, ``TpfStampSource`` and ``AperturePhotometry.photometry()``;
``plugin_files``  the baseline with files: per file ``load_tpfs([file])`` and ``tessphot('aperture', starid, TpfStampSource(...), folder,
                  datasource='tpf')``, which writes the light curve of an OK / WARNING target.
The baselines are the only way from a target pixel file to a light curve without the batched entry; they run on ``--plugin-files`` of the
files (default: all).
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

H = W = 11
ROWS = 19000


def make_files(root, n):
	"""n TPFs of 11 x 11 x 19 000 written with fitsio's own writer: one star in the middle of a noisy background, each file its own
	place on the CCD and its own ``TICID``.  Returns ``(files, catalog)``."""
	import numpy as np
	from photometry_amd import fitsio
	rng = np.random.default_rng(1)
	yy, xx = np.mgrid[0:H, 0:W]
	star = 4000.0 * np.exp(-0.5 * ((yy - 5.2)**2 + (xx - 4.9)**2) / 0.81) / (2 * np.pi * 0.81)
	flux = (star[None] * (1 + 1e-3 * rng.normal(size=ROWS))[:, None, None] + rng.normal(0.0, 4.0, size=(ROWS, H, W))).astype('float32')
	err = np.sqrt(np.abs(flux) + 116.0).astype('float32')
	bkg = np.full((ROWS, H, W), 100.0, dtype='float32')
	quality = np.zeros(ROWS, dtype='int32')
	quality[rng.random(ROWS) < 0.02] = 32
	image = lambda name, fmt, array: {'name': name, 'format': f'{H * W}{fmt}', 'array': array, 'dim': (W, H)} # noqa: E731
	files, cat = [], {'starid': [], 'tmag': [], 'row': [], 'column': []}
	for k in range(n):
		c1p, c2p = 100 + 30 * (k % 60), 100 + 30 * (k // 60)
		cols = [{'name': 'TIME', 'format': 'D', 'array': 1683.35 + 1e-4 * k + np.arange(ROWS) * (120.0 / 86400.0)}, {'name': 'TIMECORR', 'format': 'E', 'array': np.full(ROWS, 3e-3, dtype='float32')},
			{'name': 'CADENCENO', 'format': 'J', 'array': np.arange(ROWS, dtype='int32')}, image('RAW_CNTS', 'J', flux.astype('int32')), image('FLUX', 'E', flux * np.float32(1 + 0.01 * k)),
			image('FLUX_ERR', 'E', err), image('FLUX_BKG', 'E', bkg), image('FLUX_BKG_ERR', 'E', bkg * np.float32(0.01)),
			{'name': 'QUALITY', 'format': 'J', 'array': quality}, {'name': 'POS_CORR1', 'format': 'E', 'array': np.zeros(ROWS, dtype='float32')},
			{'name': 'POS_CORR2', 'format': 'E', 'array': np.zeros(ROWS, dtype='float32')}]
		path = os.path.join(root, 'tess2019199201929-s0014-%016d-0150-s_tp.fits' % (1000 + k))
		fitsio.write(path, [fitsio.primary_hdu([fitsio.card('TELESCOP', 'TESS'), fitsio.card('SECTOR', 14), fitsio.card('CAMERA', 1), fitsio.card('CCD', 1), fitsio.card('DATA_REL', 35),
				fitsio.card('TICID', 1000 + k)]),
			fitsio.bintable_hdu('PIXELS', cols, [fitsio.card('TIMEDEL', 120.0 / 86400.0)]),
			fitsio.image_hdu('APERTURE', np.ones((H, W), dtype='int32'), [fitsio.card('CRVAL1P', c1p), fitsio.card('CRVAL2P', c2p)])])
		files.append(path)
		cat['starid'].append(1000 + k)
		cat['tmag'].append(11.5)
		cat['row'].append(c2p - 1 + 5.2)
		cat['column'].append(c1p - 1 + 4.9)
	catalog = {'starid': np.array(cat['starid'], dtype='int64'), 'tmag': np.array(cat['tmag'], dtype='float32'), 'row': np.array(cat['row'], dtype='float32'),
		'column': np.array(cat['column'], dtype='float32')}
	return files, catalog


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--files', type=int, default=16, help='synthetic TPFs (46.5 MB each; few enough for the page cache)')
	ap.add_argument('--plugin-files', type=int, default=None, help='files of the per-file baselines (default: all)')
	ap.add_argument('--repeats', type=int, default=3)
	ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory, removed afterwards)')
	ap.add_argument('--out', default=None)
	ap.add_argument('--compress', choices=('zlib', 'device'), nargs='+', default=['zlib'], help="how the light-curve files of the batch are compressed (one run of the step each)")
	ap.add_argument('--compresslevel', type=int, nargs='+', default=[9], help="gzip's levels with --compress zlib (one run of the step each)")
	ap.add_argument('--table', choices=('host', 'device'), nargs='+', default=['host'], help="who writes the LIGHTCURVE data units; 'device' runs with --compress device only")
	ap.add_argument('--skip-baselines', action='store_true', help='stop behind the batched entry: no per-file runs')
	a = ap.parse_args()
	from photometry_amd import tpf, tessphot, tessphot_tpfs, lcfile, STATUS
	from photometry_amd.device import Context
	from photometry_amd.plugins import AperturePhotometry

	def emit(res):
		print(json.dumps(res), flush=True)
		if a.out:
			with open(a.out, 'a') as fh:
				fh.write(json.dumps(res) + '\n')

	with tempfile.TemporaryDirectory(dir=a.dir) as root, Context(0) as ctx:
		files, catalog = make_files(root, a.files)
		N = len(files)
		out_dir = os.path.join(root, 'lc')
		file_bytes = sum(os.path.getsize(f) for f in files)
		for ld in tpf.load_tpfs(ctx, files):                                  # warm-up: page cache, code objects, the allocation cache
			ld.free()

		def best_of(fn, repeats=a.repeats):
			times, last = [], None
			for _ in range(repeats):
				t0 = time.perf_counter()
				last = fn()
				times.append(time.perf_counter() - t0)
			return min(times), times, last

		# ---- the loaders alone ----
		def load():
			loaded = tpf.load_tpfs(ctx, files)
			ctx.sync()
			for ld in loaded:
				ld.free()
		t, times, _ = best_of(load)
		emit({'step': 'load', 'files': N, 'file_bytes': file_bytes, 'files_per_s': N / t, 'GB_per_s': file_bytes / t / 1e9, 'all_s': times})

		def groups():
			grp, _index = tpf.load_tpf_groups(ctx, files)
			ctx.sync()
			n = len(grp)
			for g in grp:
				g.free()
			return n
		t, times, n_groups = best_of(groups)
		emit({'step': 'groups', 'files': N, 'groups': n_groups, 'files_per_s': N / t, 'GB_per_s': file_bytes / t / 1e9, 'all_s': times})

		# ---- the batched entry ----
		def batch(folder=None, compress='zlib', level=9, table='host'):
			status = []
			for res in tessphot_tpfs(ctx, files, catalog, output_folder=folder, version=6 if folder else None, compress=compress, compresslevel=level, table=table):
				status += [res[i].status for i in range(len(res))]
			return status
		batch()                                                               # warm-up
		t, times, status = best_of(batch)
		n_ok = sum(s in (STATUS.OK, STATUS.WARNING) for s in status)
		emit({'step': 'batch', 'files': N, 'ok_or_warning': n_ok, 'files_per_s': N / t, 'ms_per_file': t / N * 1e3, 'all_s': times})

		spent = {}
		save = lcfile.save_tpf_lightcurves

		def timed_save(*args, **kwargs):
			return save(*args, timings=spent, **kwargs)
		lcfile.save_tpf_lightcurves = timed_save

		for compress, table, level in [(c, t, l) for c in a.compress for t in (a.table if c == 'device' else ['host']) for l in (a.compresslevel if c == 'zlib' else a.compresslevel[:1])]:
			def batch_files():
				shutil.rmtree(out_dir, ignore_errors=True)
				spent.clear()
				return batch(out_dir, compress, level, table)
			batch_files()                                                     # warm-up of the writer (the device path: code object, buffers)
			t, times, status = best_of(batch_files)
			written = len(os.listdir(out_dir))
			deflate_kernels = None
			if compress == 'device':                                          # once more under the kernel profile
				ctx.profile(True)
				ctx.profile_reset()
				batch_files()
				ctx.sync()
				deflate_kernels = {k: v for k, v in ctx.profile_report().items() if 'deflate' in k or 'tp_lc_' in k}
				ctx.profile(False)
			emit({'step': 'batch_files', 'files': N, 'written': written, 'lc_bytes': sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)),
				'files_per_s': N / t, 'ms_per_file': t / N * 1e3, 'worker_build_s': spent.get('build'), 'worker_gzip_s': spent.get('gzip'),
				'workers': min(lcfile.MAX_WORKERS, os.cpu_count() or 1), 'all_s': times, 'compress': compress, 'table': table, 'table_s': spent.get('table'), 'place_s': spent.get('place'), 'compresslevel': level if compress == 'zlib' else None,
				'worker_write_s': spent.get('write'), 'gzip_parts_s': spent.get('gzip_parts'), 'deflate_kernels': deflate_kernels})
		lcfile.save_tpf_lightcurves = save
		if a.skip_baselines:
			return

		# ---- the per-file baselines ----
		some = files[:a.plugin_files] if a.plugin_files else files
		ids = [1000 + k for k in range(len(some))]

		def plugin():
			status = []
			for path, starid in zip(some, ids):
				(ld,) = tpf.load_tpfs(ctx, [path])
				with AperturePhotometry(starid, tpf.TpfStampSource(ld, catalog), None, datasource='tpf', ctx=ctx) as pho:
					pho.photometry()
					status.append(pho.status)
				ld.free()
			return status
		plugin()                                                              # warm-up
		t, times, status = best_of(plugin, max(1, a.repeats - 1))
		emit({'step': 'plugin', 'files': len(some), 'ok_or_warning': sum(s in (STATUS.OK, STATUS.WARNING) for s in status), 'files_per_s': len(some) / t,
			'ms_per_file': t / len(some) * 1e3, 'all_s': times})

		def plugin_files():
			shutil.rmtree(out_dir, ignore_errors=True)
			status = []
			for path, starid in zip(some, ids):
				(ld,) = tpf.load_tpfs(ctx, [path])
				pho = tessphot('aperture', starid, tpf.TpfStampSource(ld, catalog), out_dir, datasource='tpf', ctx=ctx, version=6)
				status.append(pho.status)
				ld.free()
			return status
		t, times, status = best_of(plugin_files, max(1, a.repeats - 1))
		emit({'step': 'plugin_files', 'files': len(some), 'written': len(os.listdir(out_dir)), 'files_per_s': len(some) / t, 'ms_per_file': t / len(some) * 1e3, 'all_s': times})
	return 0


if __name__ == '__main__':
	sys.exit(main())
