# -*- coding: utf-8 -*-
"""
What the tests of the light-curve table packer share (tests/test_lctable_rules_host.py, tests/test_gpu_lctable.py): the cases -- the
smallest inputs at which each rule of photometry_amd/csrc/lctable_rules.h can go wrong --, what the host path writes for them
(``fitsio.bintable_hdu`` of the 14 columns, ``fitsio._sum32``), and the host driver tests/hostsim/lctable_rules_host.cpp built with
AddressSanitizer and UBSan.
"""
import os
import subprocess
import numpy as np
import conftest
from photometry_amd import fitsio, lcfile

CSRC = os.path.join(conftest.ROOT, 'photometry_amd', 'csrc')
SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'lctable_rules_host.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'lctable_rules_host')
ROW = 96
N_ROWS = (0, 1, 2, 29, 30, 31, 63, 64, 65, 130)
GUARD = 64                                     # bytes in front of, between and behind the targets' ranges

#: float64 bit patterns that a floating-point move could change, and the plain extremes
F64_BITS = np.array([0xFFF8000000000123, 0x7FF0000000000001, 0xFFF4000000000000, 0x7FF8000000000000, 0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF,
	0x7FF0000000000000, 0xFFF0000000000000, 0x7FEFFFFFFFFFFFFF, 0x0010000000000000, 0x3FF0000000000000], dtype='uint64')
#: timecorr values: float32 ties to even (down and up), just above and below a tie, overflow to inf by magnitude and by rounding, the
#: largest float32, float32 denormals with their ties, below half the smallest denormal, zeros, inf, NaNs with sign and payload
TIMECORR = np.concatenate([np.array([1 + 2.0**-24, 1 + 3 * 2.0**-24, 1 + 2.0**-24 + 2.0**-40, 1 + 2.0**-24 - 2.0**-40, -(1 + 2.0**-24), 3.5e38, -3.5e38, 1e300,
	float(np.finfo('float32').max), float(np.finfo('float32').max) * (1 + 2.0**-25), float(np.finfo('float32').max) * (1 + 2.0**-26), 1e-40, 2.0**-149, 2.0**-150, 1.5 * 2.0**-149,
	2.5 * 2.0**-149, 2.0**-150 * (1 + 2.0**-30), 1e-46, -1e-46, 2.0**-126 * (1 - 2.0**-25), 0.0, -0.0, np.inf, -np.inf, 1.234e-3]),
	np.array([0xFFF8000000000123, 0x7FF0000020000001, 0x7FF0000000000001], dtype='uint64').view('float64')])
I32 = np.array([-2**31, 2**31 - 1, -1, 0, 1, 0x55AA55AA, -0x55AA55AA], dtype='int32')


def build_driver():
	"""The driver, compiled once per run of the suite (``-fno-sanitize-recover``: a report ends the program)."""
	os.makedirs(OUT_DIR, exist_ok=True)
	deps = [SRC, os.path.join(CSRC, 'lctable_rules.h'), os.path.join(CSRC, 'fits_rules.h')]
	if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
		subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-I' + CSRC, SRC, '-o', OUT], check=True)
	return OUT


def drive(text):
	r = subprocess.run([build_driver()], input=text, capture_output=True, text=True)
	assert r.returncode == 0 and 'FAILED' not in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
	return r.stdout.splitlines()


class Case(object):
	"""One call of ``tp_lc_table_pack``: the arrays at exactly the size the strides make a call read, the strides, the kept rows."""

	def __init__(self, name, n_targets, T, rows=None, shared=True, extra=0, quality=True, pos_corr=True, special=False, seed=0):
		rng = np.random.default_rng(1000 + seed)
		self.name, self.n_targets, self.T = name, n_targets, T
		self.rows = None if rows is None else np.asarray(rows, dtype='int32')
		self.n_rows = T if rows is None else len(self.rows)
		S = T + extra                                                   # a per-target stride, larger than T with `extra`
		span = (n_targets - 1) * S + T

		def f64(n, scale=1.0, offset=0.0):
			a = rng.normal(size=n) * scale + offset
			if special:
				a.view('uint64')[rng.choice(n, min(n, len(F64_BITS)), replace=False)] = F64_BITS[:min(n, len(F64_BITS))]
			return a

		def i32(n):
			a = rng.integers(-2**31, 2**31, n, dtype='int64').astype('int32')
			if special:
				a[rng.choice(n, min(n, len(I32)), replace=False)] = I32[:min(n, len(I32))]
			return a
		vec = T if shared else span
		self.stride = 0 if shared else S
		self.time = f64(vec, 10.0, 1500.0)
		self.timecorr = f64(vec, 1e-3)
		if special:
			self.timecorr[rng.choice(vec, min(vec, len(TIMECORR)), replace=False)] = TIMECORR[:min(vec, len(TIMECORR))]
		self.cadenceno = i32(vec)
		self.pixel_quality = i32(vec)
		self.lc_target_stride = S
		self.lc_plane_stride = n_targets * S + (extra and 3)
		self.lc = f64(4 * self.lc_plane_stride + span, 100.0, 1e4)
		self.quality_stride = S
		self.quality = i32(span) if quality else None
		self.pos_corr_stride = 2 * S
		self.pos_corr = f64((n_targets - 1) * 2 * S + 2 * T, 0.01) if pos_corr else None
		# where the targets' data units go: guards in front, between and behind, the targets not in index order
		unit = fitsio._padded(self.n_rows * ROW)
		order = list(range(n_targets))[::-1]
		self.offsets = np.zeros(n_targets, dtype='uint64')
		at = GUARD
		for i in order:
			self.offsets[i] = at
			at += unit + GUARD
		self.capacity = at
		self.unit = unit

	def kept(self):
		return np.arange(self.n_rows) if self.rows is None else self.rows.astype('int64')

	def columns(self, i):
		"""The 14 columns of target ``i`` with their arrays, as the host path hands them to ``fitsio.bintable_hdu``."""
		k = self.kept()
		n = len(k)
		v = i * self.stride + k
		lc = [self.lc[p * self.lc_plane_stride + i * self.lc_target_stride + k] for p in range(5)]
		zeros = np.zeros(n)
		arrays = {'TIME': self.time[v], 'TIMECORR': self.timecorr[v], 'CADENCENO': self.cadenceno[v], 'FLUX_RAW': lc[0], 'FLUX_RAW_ERR': lc[1], 'FLUX_BKG': lc[2],
			'FLUX_CORR': np.full(n, np.nan), 'FLUX_CORR_ERR': np.full(n, np.nan),
			'QUALITY': self.quality[i * self.quality_stride + k] if self.quality is not None else np.zeros(n, dtype='int32'), 'PIXEL_QUALITY': self.pixel_quality[v],
			'MOM_CENTR1': lc[3], 'MOM_CENTR2': lc[4],
			'POS_CORR1': self.pos_corr[i * self.pos_corr_stride + 2 * k] if self.pos_corr is not None else zeros,
			'POS_CORR2': self.pos_corr[i * self.pos_corr_stride + 2 * k + 1] if self.pos_corr is not None else zeros}
		return [dict(c, array=arrays[c['name']]) for c in lcfile.table_columns()]

	def expected(self):
		"""``(buffer bytes, datasums)``: 0xA5 everywhere but the data units ``fitsio.bintable_hdu`` gives."""
		buf = np.full(self.capacity, 0xA5, dtype='uint8')
		sums = []
		with np.errstate(over='ignore', invalid='ignore', under='ignore'):
			for i in range(self.n_targets):
				hdu = fitsio.bintable_hdu('LIGHTCURVE', self.columns(i), ())
				data = hdu[len(hdu) - self.unit:] if self.unit else b''
				assert len(data) == self.unit
				buf[int(self.offsets[i]):int(self.offsets[i]) + self.unit] = np.frombuffer(data, dtype='uint8')
				sums.append(fitsio._sum32(data) if data else 0)
		return buf.tobytes(), np.array(sums, dtype='uint64')

	def arrays(self):
		"""The source arrays in the driver's order (``None``: a null pointer)."""
		return [self.time, self.timecorr, self.cadenceno, self.pixel_quality, self.lc, self.quality, self.pos_corr]

	def strides(self):
		return [self.stride, self.stride, self.stride, self.stride, self.lc_plane_stride, self.quality_stride, self.pos_corr_stride]


def cases():
	"""name -> Case, in a fixed order."""
	out = {}

	def add(*args, **kw):
		out[args[0]] = Case(*args, seed=len(out), **kw)
	for n in N_ROWS:
		add(f'rows_{n}', 1, max(n, 1), rows=np.arange(n), special=n >= 29)
		add(f'rows_{n}_x3', 3, max(n, 1), rows=np.arange(n), shared=False, extra=5, special=n >= 29)
	add('no_list_65', 3, 65, special=True)                                  # d_rows null: all cadences
	add('dropped_first', 3, 66, rows=np.arange(1, 66), special=True)
	add('dropped_last', 3, 66, rows=np.arange(65), shared=False)
	add('dropped_middle', 3, 66, rows=np.delete(np.arange(66), 31), shared=False, extra=7, special=True)
	add('dropped_three', 1, 133, rows=np.delete(np.arange(133), [0, 64, 132]), special=True)
	add('per_target_tight', 3, 31, shared=False, special=True)              # per-target strides equal to T
	add('no_quality', 3, 31, quality=False, special=True)
	add('no_pos_corr', 3, 31, pos_corr=False, shared=False, extra=1, special=True)
	add('neither', 1, 64, quality=False, pos_corr=False)
	add('five_tiles', 2, 300, rows=np.arange(10, 300), shared=False, extra=2, special=True)   # more than one workgroup per target
	return out


def host_pack(tmp, case, null_mask=0, misalign_mask=0, name=None, **over):
	"""One ``pack`` command: ``('ok', buffer bytes, datasums)`` or ``('refused', message)``; the output file must be absent after a refusal.
	``over``: n_targets, T, n_rows, offsets, capacity, strides (list), has_rows in place of the case's."""
	name = name or case.name
	inp, out = os.path.join(str(tmp), name + '.in'), os.path.join(str(tmp), name + '.out')
	arrays = case.arrays()
	with open(inp, 'wb') as fh:
		for a in arrays:
			if a is not None:
				fh.write(a.tobytes())
		if case.rows is not None:
			fh.write(case.rows.tobytes())
	if os.path.exists(out):
		os.remove(out)
	strides = over.get('strides', case.strides())
	words = [inp, out, over.get('n_targets', case.n_targets), over.get('T', case.T), over.get('n_rows', case.n_rows), over.get('has_rows', int(case.rows is not None))]
	for k, a in enumerate(arrays):
		words += [-1 if a is None else len(a), strides[k]]
		if k == 4:
			words.append(over.get('lc_target_stride', case.lc_target_stride))
	offsets = over.get('offsets', case.offsets)
	capacity = over.get('capacity', case.capacity)
	words += [capacity, null_mask, misalign_mask] + [int(o) for o in offsets]
	lines = drive('pack ' + ' '.join(str(w) for w in words) + '\n')
	if lines[0].startswith('refused '):
		assert not os.path.exists(out)
		return 'refused', lines[0][len('refused '):]
	assert lines[0] == 'ok', lines
	with open(out, 'rb') as fh:
		blob = fh.read()
	n = over.get('n_targets', case.n_targets)
	assert len(blob) == capacity + 8 * n
	return 'ok', blob[:capacity], np.frombuffer(blob[capacity:], dtype='uint64')


def host_place(tmp, src, dst_capacity, segments, null_mask=0, misalign_mask=0, name='place', src_capacity=None):
	"""One ``place`` command over the bytes ``src``: ``('ok', destination bytes)`` or ``('refused', message)``."""
	inp, out = os.path.join(str(tmp), name + '.in'), os.path.join(str(tmp), name + '.out')
	with open(inp, 'wb') as fh:
		fh.write(src)
	if os.path.exists(out):
		os.remove(out)
	flat = ' '.join(f'{a} {b} {c}' for a, b, c in segments)
	lines = drive(f'place {inp} {out} {len(src) if src_capacity is None else src_capacity} {dst_capacity} {len(segments)} {null_mask} {misalign_mask} {flat}\n')
	if lines[0].startswith('refused '):
		assert not os.path.exists(out)
		return 'refused', lines[0][len('refused '):]
	assert lines[0] == 'ok', lines
	with open(out, 'rb') as fh:
		return 'ok', fh.read()


def place_expected(src, dst_capacity, segments):
	dst = np.full(dst_capacity, 0xA5, dtype='uint8')
	s = np.frombuffer(src, dtype='uint8')
	for a, b, c in segments:
		dst[b:b + c] = s[a:a + c]
	return dst.tobytes()


def place_cases():
	"""name -> (source bytes, destination capacity, [(src offset, dst offset, length)]): 1 and 5 segments of 16, 2880 and 5760 bytes
	with guard bytes around every destination range, the segments not in address order."""
	rng = np.random.default_rng(77)
	out = {}
	for length in (16, 2880, 5760):
		src = rng.integers(0, 256, 5 * length + 32, dtype='uint8').tobytes()
		out[f'one_{length}'] = (src, length + 64, [(16, 32, length)])
		segs = [(16 + k * length, 16 + (4 - k) * (length + 16), length) for k in range(5)]
		out[f'five_{length}'] = (src, 16 + 5 * (length + 16), segs)
	src = rng.integers(0, 256, 2880 + 5760 + 16, dtype='uint8').tobytes()
	out['mixed_with_empty'] = (src, 16 + 16 + 5760 + 16 + 2880 + 16 + 16, [(0, 16 + 5760 + 16, 2880), (2880, 16, 5760), (0, 0, 0), (2880 + 5760, 16 + 5760 + 16 + 2880 + 16, 16)])
	return out
