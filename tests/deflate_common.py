# -*- coding: utf-8 -*-
"""
What the tests of the DEFLATE encoder share (tests/test_deflate_rules_host.py, tests/test_gpu_deflate.py): the case inputs -- the
smallest at which each rule of photometry_amd/csrc/deflate_rules.h can go wrong --, the host driver tests/hostsim/deflate_rules_host.cpp
built with AddressSanitizer and UBSan, and the reading of a call's result: every stream inflated by zlib.
"""
import os
import subprocess
import zlib
import numpy as np
import conftest

CSRC = os.path.join(conftest.ROOT, 'photometry_amd', 'csrc')
SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'deflate_rules_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'deflate_rules_host')
C = 16384                                      # TP_DEFLATE_CHUNK (the driver's `chunk` command is held to it)
LENGTHS = (0, 1, 2, 3, 4, 257, 258, 259, 260, C - 1, C, C + 1, 2 * C + 5)
STORED, FIXED, DYNAMIC = 0, 1, 2


def build_driver():
	"""The driver, compiled once per run of the suite (``-fno-sanitize-recover``: a report ends the program)."""
	os.makedirs(OUT_DIR, exist_ok=True)
	deps = [SRC, os.path.join(CSRC, 'deflate_rules.h'), os.path.join(CSRC, 'fits_rules.h')]
	if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
		subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-I' + CSRC, SRC, '-o', OUT], check=True)
	return OUT


def drive(text):
	r = subprocess.run([build_driver()], input=text, capture_output=True, text=True)
	assert r.returncode == 0 and 'FAILED' not in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
	return r.stdout.splitlines()


def offsets_of(blobs):
	return np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype('uint64')


def host_deflate(tmp, blobs, out_capacity=-1, work_bytes=-1, null_mask=0, misalign_mask=0, n_streams=None, offsets=None, name='call'):
	"""One ``deflate`` command: ``('ok', packed bytes, ends, crcs, forms, ll lengths per chunk or None)`` or ``('refused', message)``;
	the output file must be absent after a refusal."""
	inp, out = os.path.join(str(tmp), name + '.in'), os.path.join(str(tmp), name + '.out')
	with open(inp, 'wb') as fh:
		fh.write(b''.join(blobs))
	if os.path.exists(out):
		os.remove(out)
	offsets = offsets_of(blobs) if offsets is None else offsets
	n_streams = len(blobs) if n_streams is None else n_streams
	lines = drive(f"deflate {inp} {out} {n_streams} {' '.join(str(int(o)) for o in offsets)} {out_capacity} {work_bytes} {null_mask} {misalign_mask}\n")
	if lines[0].startswith('refused '):
		assert not os.path.exists(out)
		return 'refused', lines[0][len('refused '):]
	head = lines[0].split()
	assert head[0] == 'ok' and head[1] == 'chunks' and head[3] == 'total', lines[0]
	n, total = int(head[2]), int(head[4])
	ends, crcs, forms, lens = [], [], [], []
	for line in lines[1:]:
		w = line.split()
		if w[0] == 'chunk':
			ends.append(int(w[1])); crcs.append(int(w[2])); forms.append(int(w[3])); lens.append(None)
		else:
			assert w[0] == 'll'
			lens[-1] = [int(v) for v in w[1:]]
	assert len(ends) == n
	with open(out, 'rb') as fh:
		packed = fh.read()
	assert len(packed) == total == (ends[-1] if n else 0)
	return 'ok', packed, np.array(ends, dtype='uint64'), np.array(crcs, dtype='uint32'), forms, lens


def chunks_of(blob):
	return [blob[k:k + C] for k in range(0, len(blob), C)]


def check_streams(blobs, packed, ends, crcs):
	"""Every stream of a call inflates to its input, every chunk's CRC is zlib's, every chunk is within its bound."""
	c, begin = 0, 0
	for b in blobs:
		pieces = chunks_of(b)
		end = int(ends[c + len(pieces) - 1]) if pieces else begin
		d = zlib.decompressobj(-15)
		got = d.decompress(packed[begin:end] + b'\x03\x00')
		assert d.eof and not d.unused_data and got == b, (len(b), len(got))
		at = begin
		for k, piece in enumerate(pieces):
			assert int(crcs[c + k]) == zlib.crc32(piece)
			assert int(ends[c + k]) - at <= len(piece) + 5
			at = int(ends[c + k])
		c += len(pieces)
		begin = end
	assert c == len(ends) and begin == len(packed)


def fibonacci(n):
	f = [1, 1]
	while len(f) < n:
		f.append(f[-1] + f[-2])
	return f[:n]


def cases():
	"""name -> bytes, in a fixed order."""
	rng = np.random.default_rng(20)
	rand = lambda n: rng.integers(0, 256, n, dtype='uint8').tobytes() # noqa: E731
	out = {}
	for n in LENGTHS:
		out[f'zeros_{n}'] = bytes(n)                                   # distance-1 runs, length-258 chains and their remainders
		out[f'ramp_{n}'] = (np.arange(n) % 251).astype('uint8').tobytes()
		out[f'random_{n}'] = rand(n)
	block = rand(C // 2 - 1)
	out['far'] = block + block                                         # a match at distance C // 2 - 1
	out['far_end'] = block + rand(2) + block                           # the copy pushed to the end of the chunk
	pattern = rand(100)
	out['boundary'] = rand(C - 99) + pattern + pattern                 # the repeat begins one byte behind the chunk boundary
	out['one_value'] = b'\x07' * 1000
	out['two_values'] = rng.choice(np.array([3, 200], dtype='uint8'), 3000).tobytes()
	out['all_values'] = rng.permutation(256).astype('uint8').tobytes()
	# literal counts along the Fibonacci numbers: the longest run of them that fits a chunk (19 symbols, 10 945 bytes; the 22
	# symbols at which an unlimited code is 21 bits deep are 46 367 bytes -- those counts go to the code builder directly)
	fib = fibonacci(19)
	out['fibonacci'] = rng.permutation(np.repeat(np.arange(19, dtype='uint8') * 13, fib)).tobytes()
	# header coding: the literals 101 .. 239 unused (138 + 1 zero lengths), seven literals of one length between two of another --
	# of another: 0 and 8 are rare, 1 .. 7 as frequent as the other 93 literals -- enough of those that no four bytes repeat
	counts = {s: 150 for s in list(range(0, 101)) + [240]}
	counts.update({0: 8, 8: 8})
	out['header_runs'] = rng.permutation(np.repeat(np.array(list(counts), dtype='uint8'), list(counts.values()))).tobytes()
	return out


def lightcurve_table(n_bytes=600000, rows=19000):
	"""The first ``n_bytes`` bytes of a 19 000-row light-curve file as ``lcfile.lightcurve_hdus`` builds it from noise series: the
	recipe of tests/test_lcfile_host.py (``_lightcurve``, ``_images``, ``_hdus``), restated."""
	from photometry_amd import lcfile
	H, W, stamp = 5, 6, (100, 105, 200, 206)
	time = 1700.0 + np.arange(rows) / 720
	rng = np.random.default_rng(1)
	n = rows
	lc = {'time': np.asarray(time, dtype='float64'), 'timecorr': rng.normal(size=n) * 1e-3, 'cadenceno': np.arange(n, dtype='int32') + 4700,
		'quality': (np.arange(n) % 3 == 0).astype('int32') * 32, 'flux': rng.normal(1e4, 10, n), 'flux_err': rng.uniform(1, 2, n),
		'flux_background': rng.normal(100, 1, n), 'pos_centroid': rng.normal(size=(n, 2)) + (203.0, 102.0), 'pos_corr': rng.normal(size=(n, 2)) * 0.01}
	rng = np.random.default_rng(2)
	sumimage = rng.uniform(10, 1e4, (H, W))
	sumimage[0, 0] = np.nan
	mask = np.zeros((H, W), dtype=bool)
	mask[1:4, 2:5] = True
	bpu = np.zeros((H + 4, W + 4), dtype=bool)
	bpu[2, 2:] = True
	aperture = lcfile.aperture_with_masks(lcfile.ffi_aperture(sumimage, stamp, bpu, 98, 198), mask, mask)
	hdus = lcfile.lightcurve_hdus({'tmag': 9.25}, 261136679, 14, 2, 3, 120, 20, 6, 'aperture', 8, {'CRMITEN': True, 'CRBLKSZ': 10, 'CRSPOC': False, 'DATA_REL': 20}, 900, 720,
		{'AP_CONT': (0.0125, 'AP contamination'), 'KP_WS': (True, 'K2P2 watershed segmentation')}, lc, np.zeros(n, dtype='int32'), sumimage, aperture, lcfile.image_cards(stamp))
	blob = b''.join(hdus)
	assert len(blob) > n_bytes
	return blob[:n_bytes]


def zlib_raw(blob, level, strategy=zlib.Z_DEFAULT_STRATEGY):
	c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
	return c.compress(blob) + c.flush()
