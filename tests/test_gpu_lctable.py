# -*- coding: utf-8 -*-
"""
``tp_lc_table_pack`` and ``tp_lc_place`` on the device (csrc/lctable.hip): the cases of tests/lctable_common.py -- those of the host
test -- through the library into an output buffer pre-filled with 0xA5.  Every byte inside a target's range equals the data unit of
``fitsio.bintable_hdu``, every byte outside keeps its fill, every DATASUM equals ``fitsio._sum32``, a second call gives the same
bytes; a refused call returns ``TP_ERR_INVALID`` and leaves the buffer untouched; the ctypes mirror of ``tp_lc_table_src`` has the
layout a C compiler gives the header's struct.  Byte for byte: there is no tolerance.
"""
import ctypes
import os
import shutil
import subprocess
import numpy as np
import pytest
import conftest
import lctable_common as lc

pytestmark = pytest.mark.gpu

TP_ERR_INVALID = -1
CASES = lc.cases()


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def test_the_error_code_is_the_header_s():
	import re
	text = open(os.path.join(conftest.ROOT, 'include', 'tessphot_hip.h')).read()
	assert int(re.search(r'#define\s+TP_ERR_INVALID\s+(-?\d+)', text).group(1)) == TP_ERR_INVALID


class DeviceCall(object):
	"""The arrays of a case in device memory and one call of ``tp_lc_table_pack`` over them; ``over``: values in place of the case's."""

	def __init__(self, ctx, case):
		from photometry_amd._lib import tp_lc_table_src
		self.ctx, self.case = ctx, case
		self.held = [None if a is None else ctx.array(a) for a in case.arrays()]
		self.d_rows = None if case.rows is None or len(case.rows) == 0 else ctx.array(case.rows)
		p = [None if d is None else d.ptr for d in self.held]
		s = case.strides()
		self.src = tp_lc_table_src(p[0], s[0], p[1], s[1], p[2], s[2], p[3], s[3], p[4], s[4], case.lc_target_stride, p[5], s[5], p[6], s[6])
		self.d_out = ctx.empty(max(case.capacity, 16), 'uint8')
		self.d_sums = ctx.empty(max(case.n_targets, 1), 'uint64')

	def run(self, fill=0xA5, **over):
		ctx, case = self.ctx, self.case
		self.d_out.fill_bytes(fill)
		self.d_sums.fill_bytes(0x5A)
		no_offsets = 'offsets' in over and over['offsets'] is None
		offsets = np.ascontiguousarray(case.offsets if no_offsets else over.get('offsets', case.offsets), dtype='uint64')
		src = over.get('src', self.src)
		# (an empty row list is a pointer that is not null and never read: n_rows is 0)
		rows = over['rows'] if 'rows' in over else (self.d_rows.ptr if self.d_rows is not None else (None if case.rows is None else self.d_sums.ptr))
		rc = ctx.lib.tp_lc_table_pack(ctx.handle, ctypes.byref(src) if src is not None else None, rows, over.get('n_rows', case.n_rows), over.get('T', case.T),
			over.get('n_targets', case.n_targets), over['out'] if 'out' in over else self.d_out.ptr, None if no_offsets else offsets.ctypes.data,
			over.get('capacity', case.capacity), over['sums'] if 'sums' in over else self.d_sums.ptr)
		ctx.sync()
		return rc, self.d_out.to_host()[:case.capacity].tobytes(), self.d_sums.to_host()[:case.n_targets]

	def free(self):
		for d in self.held + [self.d_rows, self.d_out, self.d_sums]:
			if d is not None:
				d.free()


@pytest.mark.parametrize('name', list(CASES))
def test_bytes_and_sums_are_the_host_path_s(ctx, name):
	case = CASES[name]
	want, sums = case.expected()
	call = DeviceCall(ctx, case)
	try:
		rc, got, got_sums = call.run()
		assert rc == 0, ctx.lib.tp_last_error(ctx.handle)
		if got != want:
			a, b = np.frombuffer(got, dtype='uint8'), np.frombuffer(want, dtype='uint8')
			bad = np.flatnonzero(a != b)
			pytest.fail(f'{name}: {len(bad)} bytes differ, the first at {bad[0]} (offsets {case.offsets}, unit {case.unit}): {a[bad[0]]:#x} for {b[bad[0]]:#x}')
		assert np.array_equal(got_sums, sums), (got_sums, sums)
		rc, again, again_sums = call.run()                                  # a second call: the same bytes
		assert rc == 0 and again == got and np.array_equal(again_sums, got_sums)
		if case.unit:                                                       # with another fill, so that a byte the kernel skips cannot pass for written
			rc, other, _ = call.run(fill=0x3C)
			inside = np.zeros(case.capacity, dtype=bool)
			for o in case.offsets:
				inside[int(o):int(o) + case.unit] = True
			a, b = np.frombuffer(other, dtype='uint8'), np.frombuffer(want, dtype='uint8')
			assert rc == 0 and np.array_equal(a[inside], b[inside]) and np.all(a[~inside] == 0x3C)
	finally:
		call.free()


def test_the_host_composition_gives_the_same_bytes(ctx, tmp_path):
	"""Library and host driver agree on a case with dropped rows, strides above T and several tiles (both were held to numpy above)."""
	case = CASES['five_tiles']
	res = lc.host_pack(tmp_path, case)
	call = DeviceCall(ctx, case)
	try:
		rc, got, sums = call.run()
		assert rc == 0 and res[0] == 'ok' and got == res[1] and np.array_equal(sums, res[2])
	finally:
		call.free()


def _refusals(case):
	from photometry_amd._lib import tp_lc_table_src

	def without(field):
		def make(call):
			s = tp_lc_table_src.from_buffer_copy(call.src)
			setattr(s, field, None)
			return dict(src=s)
		return make
	out = [(f'null_{f}', without(f)) for f in ('time', 'timecorr', 'cadenceno', 'pixel_quality', 'lc')]

	def negative(call):
		s = tp_lc_table_src.from_buffer_copy(call.src)
		s.lc_plane_stride = -1
		return dict(src=s)
	out += [
		('null_description', lambda call: dict(src=None)),
		('null_out', lambda call: dict(out=None)),
		('null_datasum', lambda call: dict(sums=None)),
		('null_offsets', lambda call: dict(offsets=None)),
		('no_targets', lambda call: dict(n_targets=0)),
		('negative_rows', lambda call: dict(n_rows=-1)),
		('rows_above_T', lambda call: dict(n_rows=case.T + 1)),
		('T_zero', lambda call: dict(T=0, n_rows=0)),
		('rows_above_the_sum_bound', lambda call: dict(T=178956971, n_rows=178956971)),
		('negative_stride', negative),
		('offset_not_16', lambda call: dict(offsets=[8, 4000, 8000])),
		('range_leaves', lambda call: dict(capacity=3 * 64 + 3 * 5760 - 16)),
		('ranges_overlap', lambda call: dict(offsets=[64, 64 + 5760 - 16, 64 + 2 * 5760 + 64])),
		('misaligned_out', lambda call: dict(out=call.d_out.ptr + 8)),
		('misaligned_datasum', lambda call: dict(sums=call.d_sums.ptr + 4)),
		('misaligned_rows', lambda call: dict(rows=call.d_rows.ptr + 2)),
	]
	return out


def test_refusals_leave_the_buffer_untouched(ctx):
	case = CASES['rows_31_x3']
	assert case.unit == 5760 and case.n_targets == 3
	call = DeviceCall(ctx, case)
	try:
		seen = 0
		for name, make in _refusals(case):
			rc, got, sums = call.run(**make(call))
			assert rc == TP_ERR_INVALID, name
			assert b'tp_lc_table_pack' in ctx.lib.tp_last_error(ctx.handle), name
			assert got == b'\xa5' * case.capacity and np.all(sums == 0x5A5A5A5A5A5A5A5A), name
			seen += 1
		assert seen == 21
		rc, got, _ = call.run()                                             # the call as it stands is taken
		assert rc == 0 and got == case.expected()[0]
	finally:
		call.free()


def _place(ctx, src, capacity, segments, **over):
	d_src = ctx.array(np.frombuffer(src, dtype='uint8'))
	d_dst = ctx.empty(max(capacity, 16), 'uint8')
	d_dst.fill_bytes(0xA5)
	try:
		seg = np.array(segments, dtype='uint64').reshape(-1, 3)
		so, do, ln = (np.ascontiguousarray(seg[:, c]) for c in range(3))
		rc = ctx.lib.tp_lc_place(ctx.handle, None if over.get('null_src') else d_src.ptr + over.get('src_shift', 0), len(src), so.ctypes.data, do.ctypes.data,
			None if over.get('no_lengths') else ln.ctypes.data, len(seg), d_dst.ptr + over.get('dst_shift', 0), capacity)
		ctx.sync()
		return rc, d_dst.to_host()[:capacity].tobytes()
	finally:
		d_src.free()
		d_dst.free()


@pytest.mark.parametrize('name', list(lc.place_cases()))
def test_place(ctx, name):
	src, capacity, segments = lc.place_cases()[name]
	rc, got = _place(ctx, src, capacity, segments)
	assert rc == 0 and got == lc.place_expected(src, capacity, segments)
	rc, again = _place(ctx, src, capacity, segments)
	assert rc == 0 and again == got


def test_place_refusals_leave_the_buffer_untouched(ctx):
	src = bytes(range(256)) * 23                      # 5888 bytes
	good = [(0, 0, 2880), (2880, 2880, 2880)]
	for name, segments, over in (
			('src_offset_not_16', [(8, 0, 16)], {}), ('dst_offset_not_16', [(0, 8, 16)], {}), ('length_not_16', [(0, 0, 24)], {}),
			('leaves_the_source', [(2880, 0, 5888 - 2880 + 16)], {}), ('leaves_the_destination', [(0, 2880 + 16, 2880)], {}),
			('destinations_overlap', [(0, 0, 2880), (2880, 2880 - 16, 2880)], {}), ('no_segments', [], {}), ('null_src', good, dict(null_src=True)),
			('null_lengths', good, dict(no_lengths=True)), ('misaligned_src', good, dict(src_shift=8)), ('misaligned_dst', good, dict(dst_shift=8))):
		rc, got = _place(ctx, src, 5760, segments, **over)
		assert rc == TP_ERR_INVALID and got == b'\xa5' * 5760, name
		assert b'tp_lc_place' in ctx.lib.tp_last_error(ctx.handle), name
	rc, got = _place(ctx, src, 5760, good)
	assert rc == 0 and got == src[:5760]


def test_kernel_names_and_launch_counts(ctx):
	names = [ctx.lib.tp_kernel_name(k).decode() for k in range(ctx.lib.tp_kernel_count())]
	assert {'tp_lc_table_pack_kernel', 'tp_lc_table_fold_kernel', 'tp_lc_place_kernel'} <= set(names)
	case = CASES['five_tiles']
	call = DeviceCall(ctx, case)
	ctx.profile(True)
	ctx.profile_reset()
	try:
		rc, _got, _sums = call.run()
		rc2, _ = _place(ctx, bytes(2880), 2880, [(0, 0, 2880)])
		report = ctx.profile_report()
	finally:
		ctx.profile(False)
		call.free()
	assert rc == 0 and rc2 == 0
	assert report['tp_lc_table_pack_kernel'][0] == 1 and report['tp_lc_table_fold_kernel'][0] == 1 and report['tp_lc_place_kernel'][0] == 1


def test_struct_mirror_has_the_c_layout(tmp_path):
	"""``_lib.tp_lc_table_src`` against the header's struct as gcc lays it out (as tests/test_abi.py does for the other structs)."""
	from photometry_amd import _lib
	if shutil.which('gcc') is None:
		pytest.skip('no C compiler')
	header = os.path.join(conftest.ROOT, 'include', 'tessphot_hip.h')
	cls = _lib.tp_lc_table_src
	lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tessphot_hip.h"', 'int main(void) {', '	printf("size %zu\\n", sizeof(tp_lc_table_src));']
	for field, _ in cls._fields_:
		lines.append(f'	printf("{field} %zu\\n", offsetof(tp_lc_table_src, {field}));')
	lines += ['	return 0;', '}']
	src = tmp_path / 'layout.c'
	src.write_text('\n'.join(lines))
	exe = tmp_path / 'layout'
	subprocess.run(['gcc', '-I', os.path.dirname(header), str(src), '-o', str(exe)], check=True)
	out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
	assert len(out) == len(cls._fields_) + 1 == 16
	assert ctypes.sizeof(cls) == int(out['size']) == 120
	for field, _ in cls._fields_:
		assert getattr(cls, field).offset == int(out[field]), field
