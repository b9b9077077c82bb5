#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of the target-pixel-file input path (``photometry_amd.tpf.load_tpfs``, csrc/tpfin.hip) on synthetic files of
the shape of a 2-minute target (11 x 11 pixels, 19 000 rows of 2448 bytes, 46.5 MB) that sit in the page cache, beside the numpy
restatement of the conversion the path replaces.  Nothing is asserted; one JSON line per step, appended to ``--out``.

Steps, all in one process, each timed with a host clock around work that ends in a device synchronise, after one warm-up pass:
``load``      ``load_tpfs`` over all files, ``--repeats`` times: files/s, GB/s of file bytes, and the host's share spent reading
              (``stats['read_s']``) and waiting for the device (``stats['wait_s']``);
``read``      the reader alone: every file's table and APERTURE image ``readinto`` a page-locked buffer;
``transfer``  the link alone: the table's bytes from the page-locked buffer to the device (``tp_upload_cube_async``);
``unpack``    the kernels alone: ``tp_fits_datasum`` + ``tp_tpf_unpack`` per file, kernel times from ``tp_profile_get`` and the bytes
              they move over them;
``numpy``     the conversion restated: ``np.frombuffer`` with the table dtype, the three image fields to native float32 and transposed to
              ``(H, W, T)`` on one host core, then ``DeviceCube.from_host``; per file and per core.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 11
ROWS = 19000
IMAGES = ('FLUX', 'FLUX_ERR', 'FLUX_BKG')


def make_files(root, n):
	"""n TPFs of 11 x 11 x 19 000 written with fitsio's own writer (DATASUM cards included)."""
	import numpy as np
	from photometry_amd import fitsio
	rng = np.random.default_rng(1)
	flux = rng.normal(150.0, 12.0, size=(ROWS, H, W)).astype('float32')
	image = lambda name, fmt, array: {'name': name, 'format': f'{H * W}{fmt}', 'array': array, 'dim': (W, H)} # noqa: E731
	files = []
	for k in range(n):
		cols = [{'name': 'TIME', 'format': 'D', 'array': 1683.35 + np.arange(ROWS) * (120.0 / 86400.0)}, {'name': 'TIMECORR', 'format': 'E', 'array': np.full(ROWS, 3e-3, dtype='float32')},
			{'name': 'CADENCENO', 'format': 'J', 'array': np.arange(ROWS, dtype='int32')}, image('RAW_CNTS', 'J', flux.astype('int32')), image('FLUX', 'E', flux + np.float32(k)),
			image('FLUX_ERR', 'E', np.sqrt(flux)), image('FLUX_BKG', 'E', flux * np.float32(0.1)), image('FLUX_BKG_ERR', 'E', flux * np.float32(0.01)),
			{'name': 'QUALITY', 'format': 'J', 'array': np.zeros(ROWS, dtype='int32')}, {'name': 'POS_CORR1', 'format': 'E', 'array': np.zeros(ROWS, dtype='float32')},
			{'name': 'POS_CORR2', 'format': 'E', 'array': np.zeros(ROWS, dtype='float32')}]
		path = os.path.join(root, 'tess2019199201929-s0014-%016d-0150-s_tp.fits' % (1000 + k))
		fitsio.write(path, [fitsio.primary_hdu([fitsio.card('TELESCOP', 'TESS'), fitsio.card('SECTOR', 14), fitsio.card('CAMERA', 1), fitsio.card('CCD', 1), fitsio.card('DATA_REL', 35)]),
			fitsio.bintable_hdu('PIXELS', cols, [fitsio.card('TIMEDEL', 120.0 / 86400.0)]),
			fitsio.image_hdu('APERTURE', np.ones((H, W), dtype='int32'), [fitsio.card('CRVAL1P', 200), fitsio.card('CRVAL2P', 300)])])
		files.append(path)
	return files


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--files', type=int, default=16, help='synthetic TPFs (46.5 MB each)')
	ap.add_argument('--repeats', type=int, default=3)
	ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory, removed afterwards)')
	ap.add_argument('--out', default=None)
	a = ap.parse_args()
	import numpy as np
	from photometry_amd import staging, tpf
	from photometry_amd.device import Context, DeviceCube

	def emit(res):
		print(json.dumps(res), flush=True)
		if a.out:
			with open(a.out, 'a') as fh:
				fh.write(json.dumps(res) + '\n')

	with tempfile.TemporaryDirectory(dir=a.dir) as root, Context(0) as ctx:
		files = make_files(root, a.files)
		N = len(files)
		infos = [tpf.read_tpf_header(f) for f in files]
		file_bytes = sum(os.path.getsize(f) for f in files)
		for ld in tpf.load_tpfs(ctx, files):                                  # warm-up: page cache, code objects, the allocation cache
			ld.free()

		# ---- load_tpfs ----
		runs = []
		for _ in range(a.repeats):
			t0 = time.perf_counter()
			loaded = tpf.load_tpfs(ctx, files)
			ctx.sync()
			wall = time.perf_counter() - t0
			runs.append({'wall_s': wall, 'read_s': sum(ld.stats['read_s'] for ld in loaded), 'wait_s': sum(ld.stats['wait_s'] for ld in loaded)})
			for ld in loaded:
				ld.free()
		best = min(runs, key=lambda r: r['wall_s'])
		emit({'step': 'load', 'files': N, 'file_bytes': file_bytes, 'runs': runs, 'files_per_s': N / best['wall_s'], 'GB_per_s': file_bytes / best['wall_s'] / 1e9,
			'ms_per_file': best['wall_s'] / N * 1e3, 'read_share': best['read_s'] / best['wall_s'], 'wait_share': best['wait_s'] / best['wall_s']})

		# ---- the reader alone ----
		tb, apu = infos[0].table, infos[0].aperture
		span = apu.offset + apu.nbytes - tb.offset
		stage = ctx.pinned((span,), 'uint8')
		times = []
		for _ in range(a.repeats):
			t0 = time.perf_counter()
			for h in infos:
				staging.read_into(h.path, stage.array, h.table.offset, span)
			times.append(time.perf_counter() - t0)
		emit({'step': 'read', 'ms_per_file': min(times) / N * 1e3, 'GB_per_s': span * N / min(times) / 1e9, 'all_s': times})

		# ---- the link alone ----
		d_table = ctx.empty((tb.nbytes,), 'uint8')
		times = []
		for _ in range(a.repeats):
			ctx.sync()
			t0 = time.perf_counter()
			for _k in range(N):
				ctx._check(ctx.lib.tp_upload_cube_async(ctx.handle, d_table.ptr, tb.nbytes // 4, stage.ptr, tb.nbytes // 4, 1, tb.nbytes // 4))
			ctx.sync()
			times.append(time.perf_counter() - t0)
		emit({'step': 'transfer', 'ms_per_file': min(times) / N * 1e3, 'GB_per_s': tb.nbytes * N / min(times) / 1e9, 'all_s': times})

		# ---- the kernels alone ----
		cubes = [DeviceCube(ctx, 1, ROWS, H, W) for _ in IMAGES]
		d_sum = ctx.zeros((1,), 'uint64')
		offsets = (ctypes.c_int64 * 3)(*[tb.columns[c].offset for c in IMAGES])
		outs = (ctypes.c_void_p * 3)(*[c.ptr for c in cubes])

		def kernels():
			ctx._check(ctx.lib.tp_fits_datasum(ctx.handle, d_table.ptr, tb.nbytes, d_sum.ptr))
			ctx._check(ctx.lib.tp_tpf_unpack(ctx.handle, d_table.ptr, tb.row_bytes, tb.n_rows, None, ROWS, 3, ctypes.addressof(offsets), H * W, ctypes.addressof(outs), cubes[0].t_pitch))
		kernels()
		ctx.sync()
		ctx.profile(True)
		ctx.profile_reset()
		t0 = time.perf_counter()
		for _ in range(N * a.repeats):
			kernels()
		ctx.sync()
		wall = time.perf_counter() - t0
		ctx.profile(False)
		n = N * a.repeats
		kern = {k: {'launches': c, 'ms_per_file': t / n} for k, (c, t) in ctx.profile_report().items() if k.startswith(('tp_fits', 'tp_tpf'))}
		moved = {'tp_fits_datasum_kernel': tb.nbytes, 'tp_tpf_unpack_kernel': 3 * H * W * 4 * (ROWS + cubes[0].t_pitch)}
		for k, b in moved.items():
			if k in kern:
				kern[k]['GB_per_s'] = b / (kern[k]['ms_per_file'] * 1e-3) / 1e9
		emit({'step': 'unpack', 'wall_ms_per_file': wall / n * 1e3, 'kernels': kern, 'bytes_per_file': sum(moved.values())})
		stage.free()
		for c in cubes:
			c.free()

		# ---- the conversion restated in numpy, one core ----
		dt = np.dtype([(n_, c.tform[-1].replace('D', '>f8').replace('E', '>f4').replace('J', '>i4'), tuple(reversed(c.tdim)) if c.tdim else ()) for n_, c in tb.columns.items()])
		assert dt.itemsize == tb.row_bytes
		conv, up = [], []
		for _ in range(max(1, a.repeats - 1)):
			tc, tu = 0.0, 0.0
			for h in infos:
				t0 = time.perf_counter()
				blob = np.fromfile(h.path, dtype='uint8')
				rec = np.frombuffer(blob, dtype=dt, count=ROWS, offset=h.table.offset)
				host = [np.ascontiguousarray(np.moveaxis(rec[name].astype('float32'), 0, 2)) for name in IMAGES]
				t1 = time.perf_counter()
				dev = [DeviceCube.from_host(ctx, x) for x in host]
				ctx.sync()
				t2 = time.perf_counter()
				for d in dev:
					d.free()
				tc, tu = tc + (t1 - t0), tu + (t2 - t1)
			conv.append(tc)
			up.append(tu)
		emit({'step': 'numpy', 'convert_ms_per_file': min(conv) / N * 1e3, 'upload_ms_per_file': min(up) / N * 1e3,
			'files_per_s_per_core': N / (min(conv) + min(up)), 'all_convert_s': conv, 'all_upload_s': up})
	return 0


if __name__ == '__main__':
	sys.exit(main())
