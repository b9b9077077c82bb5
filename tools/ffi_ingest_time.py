#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Timing of the FFI input path (``photometry_amd.ffi.load_ffis``, csrc/fitsin.hip) on synthetic TESS-shaped files
(2078 x 2136 float32 image and uncertainty, 35.5 MB each) that sit in the page cache, beside the numpy restatement of the converter
the path replaces.  Nothing is asserted; one JSON line per step, appended to ``--out``.

Steps, all in one process, each timed with a host clock around work that ends in a device synchronise, after one warm-up pass:
``load``      ``load_ffis`` over all files, ``--repeats`` times: frames/s, GB/s of file bytes, and the host's share spent reading
              (``stats['read_s']``) and waiting for the device (``stats['wait_s']``);
``read``      the reader alone: every file's two data units ``readinto`` a page-locked buffer;
``transfer``  the link alone: the same bytes from the page-locked buffer to the device (``tp_upload_cube_async``);
``unpack``    the kernels alone: ``tp_fits_datasum`` + ``tp_fits_unpack`` of both units per frame, kernel times from ``tp_profile_get``
              and the bytes they move over them;
``numpy``     today's converter restated: ``'>f4'`` view of the file -> crop -> ``astype('float32')`` into a ``(T, R, C)`` array on one
              host core, then ``frameio.upload_group``; per frame and per core.

``--gz LEVEL`` writes the files as ``.fits.gz`` instead (``--distinct`` of them compressed, the rest copies; the compression ratio of
what was written is printed) and times these steps only, ``--inflate host device`` choosing the paths:
``load_gz``   ``load_ffis`` on the ``.gz`` files: ``inflate='host'`` (the reader thread's ``gzip``: today's path, on the first
              ``--host-files`` files) and ``inflate='device'`` at every ``--batch-files`` (0: the loader's default), frames/s;
``decoder``   ``tp_inflate`` alone on ``--decoder-files`` members already in device memory: MB/s of output in aggregate and per
              wavefront, from the kernel's time in ``tp_profile_get``.
Synthetic noise pixels compress less than real FFIs do.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (2078, 2136)
UNIT = -(-SHAPE[0] * SHAPE[1] * 4 // 2880) * 2880


def make_files(root, n):
	"""n TESS-shaped FFIs written with fitsio's own writer (DATASUM cards included)."""
	import numpy as np
	from photometry_amd import fitsio
	rng = np.random.default_rng(1)
	base = rng.normal(150.0, 12.0, size=SHAPE).astype('float32')
	err = np.sqrt(np.abs(base)).astype('float32')
	files = []
	for k in range(n):
		img = base + np.float32(k)
		cards = [fitsio.card('TSTART', 1325.3 + k / 48.0), fitsio.card('TSTOP', 1325.3 + (k + 1) / 48.0), fitsio.card('FFIINDEX', 4697 + k), fitsio.card('BARYCORR', 0.004),
			fitsio.card('DQUALITY', 0)]
		path = os.path.join(root, 'tess2018206%06d-s0001-1-1-0120-s_ffic.fits' % (45240 + k))
		fitsio.write(path, [fitsio.primary_hdu([fitsio.card('TELESCOP', 'TESS'), fitsio.card('CAMERA', 1), fitsio.card('CCD', 1)]),
			fitsio.image_hdu('CAMERA.CCD 1.1 cal', img, cards), fitsio.image_hdu('CAMERA.CCD 1.1 uncert', err)])
		files.append(path)
	return files


def compress_files(root, plain, n, level):
	"""``n`` ``.fits.gz`` files from the plain ones at zlib level ``level``: each plain file compressed once, then copied in rotation
	(the loader's work per file does not depend on the other files).  Returns the files and compressed / plain bytes."""
	import gzip
	import shutil
	made, files = [], []
	for k in range(n):
		path = os.path.join(root, 'tess2018206%06d-s0001-1-1-0120-s_ffic.fits.gz' % (45240 + k))
		if k < len(plain):
			with open(plain[k], 'rb') as src, gzip.open(path, 'wb', compresslevel=level) as dst:
				shutil.copyfileobj(src, dst, 1 << 24)
			made.append(path)
		else:
			shutil.copyfile(made[k % len(made)], path)
		files.append(path)
	return files, sum(os.path.getsize(f) for f in made) / sum(os.path.getsize(f) for f in plain)


def gz_steps(a, ctx, root, emit):
	"""``--gz``: the same loader on ``.fits.gz`` files, the host's inflate (today's path) beside the device's, and the decoder alone."""
	from photometry_amd import ffi, inflate
	plain = make_files(root, min(a.files, a.distinct))
	files, ratio = compress_files(root, plain, a.files, a.gz)
	T = len(files)
	emit({'step': 'gz_files', 'files': T, 'distinct': len(plain), 'level': a.gz, 'compression_ratio': ratio, 'gz_bytes_per_file': os.path.getsize(files[0]),
		'note': 'synthetic noise pixels: real FFIs compress further'})
	for mode in a.inflate:
		subset = files[:a.host_files] if mode == 'host' else files
		for batch in ([None] if mode == 'host' else a.batch_files):
			how = {} if mode == 'host' else {'inflate': 'device', 'batch_files': batch or None}
			ffi.load_ffis(ctx, subset[:max(2, len(subset) // 8)], **how).free()                # warm-up: page cache, code objects, the allocation cache
			runs = []
			for _ in range(a.repeats):
				t0 = time.perf_counter()
				loaded = ffi.load_ffis(ctx, subset, **how)
				ctx.sync()
				wall = time.perf_counter() - t0
				runs.append({'wall_s': wall, 'read_s': loaded.stats['read_s'], 'wait_s': loaded.stats['wait_s'], 'inflate_wait_s': loaded.stats['inflate_wait_s']})
				loaded.free()
			best = min(runs, key=lambda r: r['wall_s'])
			emit({'step': 'load_gz', 'inflate': mode, 'batch_files': batch or ('default' if mode == 'device' else None), 'files': len(subset), 'runs': runs,
				'frames_per_s': len(subset) / best['wall_s'], 'ms_per_frame': best['wall_s'] / len(subset) * 1e3})
	if 'device' in a.inflate:
		# the decoder alone: the members in device memory, one tp_inflate, kernel time from the profile
		members = [open(f, 'rb').read() for f in files[:a.decoder_files]]
		frames = [inflate.parse_member(m) for m in members]
		ctx.profile(True)
		ctx.profile_reset()
		call = inflate._Call(ctx, [memoryview(m)[b:e] for m, (b, e, _c, _i) in zip(members, frames)], [i for _b, _e, _c, i in frames])
		ctx.profile(False)
		ok = bool((call.statuses == 0).all() and all(int(c) == f[2] for c, f in zip(call.crcs, frames)))
		call.free()
		launches, ms = ctx.profile_report()['tp_inflate_kernel']
		out_bytes = sum(f[3] for f in frames)
		emit({'step': 'decoder', 'streams': len(members), 'all_ok_and_crc': ok, 'kernel_ms': ms, 'out_MB_per_s_aggregate': out_bytes / ms / 1e3,
			'out_MB_per_s_per_wavefront': max(f[3] for f in frames) / ms / 1e3, 'in_MB_per_s_aggregate': sum(len(m) for m in members) / ms / 1e3})


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--files', type=int, default=24, help='synthetic FFIs (35.5 MB each)')
	ap.add_argument('--repeats', type=int, default=3)
	ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory, removed afterwards)')
	ap.add_argument('--out', default=None)
	ap.add_argument('--gz', type=int, default=None, metavar='LEVEL', help='write the files as .fits.gz at this zlib level and time the loader on them (the steps below only)')
	ap.add_argument('--inflate', nargs='+', default=['host'], choices=['host', 'device'], help='with --gz: which inflate paths of load_ffis to time')
	ap.add_argument('--batch-files', type=int, nargs='+', default=[64, 256, 0], help="with --gz: batch_files of the device path (0: the loader's default)")
	ap.add_argument('--distinct', type=int, default=4, help='with --gz: files that are compressed; the others are copies of them')
	ap.add_argument('--host-files', type=int, default=16, help="with --gz: the first so many files go through the host's inflate (it takes a second per file)")
	ap.add_argument('--decoder-files', type=int, default=256, help='with --gz: streams of the decoder-alone launch')
	a = ap.parse_args()
	import numpy as np
	from photometry_amd import ffi, frameio, staging
	from photometry_amd.device import Context

	def emit(res):
		print(json.dumps(res), flush=True)
		if a.out:
			with open(a.out, 'a') as fh:
				fh.write(json.dumps(res) + '\n')

	if a.gz is not None:
		with tempfile.TemporaryDirectory(dir=a.dir) as root, Context(0) as ctx:
			gz_steps(a, ctx, root, emit)
		return 0
	with tempfile.TemporaryDirectory(dir=a.dir) as root, Context(0) as ctx:
		files = make_files(root, a.files)
		T = len(files)
		infos = [ffi.read_ffi_header(f) for f in files]
		file_bytes = sum(os.path.getsize(f) for f in files)
		ffi.load_ffis(ctx, files).free()                                    # warm-up: page cache, code objects, the allocation cache

		# ---- load_ffis ----
		runs = []
		for _ in range(a.repeats):
			t0 = time.perf_counter()
			loaded = ffi.load_ffis(ctx, files)
			ctx.sync()
			wall = time.perf_counter() - t0
			runs.append({'wall_s': wall, 'read_s': loaded.stats['read_s'], 'wait_s': loaded.stats['wait_s']})
			loaded.free()
		best = min(runs, key=lambda r: r['wall_s'])
		emit({'step': 'load', 'files': T, 'file_bytes': file_bytes, 'runs': runs, 'frames_per_s': T / best['wall_s'], 'GB_per_s': file_bytes / best['wall_s'] / 1e9,
			'ms_per_frame': best['wall_s'] / T * 1e3, 'read_share': best['read_s'] / best['wall_s'], 'wait_share': best['wait_s'] / best['wall_s']})

		# ---- the reader alone ----
		span = infos[0].uncert.offset + infos[0].uncert.nbytes - infos[0].image.offset
		stage = ctx.pinned((span,), 'uint8')
		times = []
		for _ in range(a.repeats):
			t0 = time.perf_counter()
			for h in infos:
				staging.read_into(h.path, stage.array, h.image.offset, span)
			times.append(time.perf_counter() - t0)
		emit({'step': 'read', 'ms_per_frame': min(times) / T * 1e3, 'GB_per_s': span * T / min(times) / 1e9, 'all_s': times})

		# ---- the link alone ----
		d_raw = ctx.empty((2, UNIT), 'uint8')
		times = []
		for _ in range(a.repeats):
			ctx.sync()
			t0 = time.perf_counter()
			for _k in range(T):
				for j, unit in enumerate((infos[0].image, infos[0].uncert)):
					ctx._check(ctx.lib.tp_upload_cube_async(ctx.handle, d_raw.ptr + j * UNIT, UNIT // 4, stage.ptr + unit.offset - infos[0].image.offset, UNIT // 4, 1, UNIT // 4))
			ctx.sync()
			times.append(time.perf_counter() - t0)
		emit({'step': 'transfer', 'ms_per_frame': min(times) / T * 1e3, 'GB_per_s': 2 * UNIT * T / min(times) / 1e9, 'all_s': times})

		# ---- the kernels alone ----
		r0, c0, R, C = ffi.TESS_WINDOW
		d_out = ctx.empty((2, R, C), 'float32')
		d_sum = ctx.zeros((2,), 'uint64')

		def kernels():
			for j in range(2):
				ctx._check(ctx.lib.tp_fits_datasum(ctx.handle, d_raw.ptr + j * UNIT, UNIT, d_sum.ptr + 8 * j))
				ctx._check(ctx.lib.tp_fits_unpack(ctx.handle, d_raw.ptr + j * UNIT, -32, SHAPE[1], SHAPE[0], r0, c0, R, C, d_out.ptr + j * R * C * 4, C))
		kernels()
		ctx.sync()
		ctx.profile(True)
		ctx.profile_reset()
		t0 = time.perf_counter()
		for _ in range(T * a.repeats):
			kernels()
		ctx.sync()
		wall = time.perf_counter() - t0
		ctx.profile(False)
		n = T * a.repeats
		kern = {k: {'launches': c, 'ms_per_frame': t / n} for k, (c, t) in ctx.profile_report().items() if k.startswith('tp_fits')}
		moved = {'tp_fits_datasum_kernel': 2 * UNIT, 'tp_fits_unpack_kernel': 2 * 2 * R * C * 4}
		for k, b in moved.items():
			if k in kern:
				kern[k]['GB_per_s'] = b / (kern[k]['ms_per_frame'] * 1e-3) / 1e9
		emit({'step': 'unpack', 'wall_ms_per_frame': wall / n * 1e3, 'kernels': kern, 'bytes_per_frame': sum(moved.values())})
		stage.free()

		# ---- today's converter restated in numpy, one core ----
		conv, up = [], []
		for _ in range(max(1, a.repeats - 1)):
			raw = np.empty((T, R, C), dtype='float32')
			raw_err = np.empty((T, R, C), dtype='float32')
			t0 = time.perf_counter()
			for k, h in enumerate(infos):
				blob = np.fromfile(h.path, dtype='uint8')
				for unit, dst in ((h.image, raw), (h.uncert, raw_err)):
					img = blob[unit.offset:unit.offset + SHAPE[0] * SHAPE[1] * 4].view('>f4').reshape(SHAPE)
					dst[k] = np.asarray(img[r0:r0 + R, c0:c0 + C], dtype='float32')
			conv.append(time.perf_counter() - t0)
			t0 = time.perf_counter()
			for x in (raw, raw_err):
				frameio.upload_group(ctx, x).free()
			ctx.sync()
			up.append(time.perf_counter() - t0)
		emit({'step': 'numpy', 'convert_ms_per_frame': min(conv) / T * 1e3, 'upload_ms_per_frame': min(up) / T * 1e3,
			'frames_per_s_per_core': T / (min(conv) + min(up)), 'all_convert_s': conv, 'all_upload_s': up})
	return 0


if __name__ == '__main__':
	sys.exit(main())
