# -*- coding: utf-8 -*-
"""
CPU checks of the light-curve table packer's device-free rules (photometry_amd/csrc/lctable_rules.h): tests/hostsim/lctable_rules_host.cpp,
built with AddressSanitizer and UBSan and run as a program, composes them serially -- every target, tile, lane and piece -- into the
bytes ``tp_lc_table_pack`` and ``tp_lc_place`` write, with source, LDS and output buffers of exactly the size a call may touch.  Every
target's bytes are held to the data unit of ``fitsio.bintable_hdu`` and its sum to ``fitsio._sum32``, byte for byte; every byte outside
the targets' ranges keeps its fill.  The cases (tests/lctable_common.py) are the smallest at which each rule can go wrong.
"""
import subprocess
import numpy as np
import pytest
import lctable_common as lc

CASES = lc.cases()


def test_header_compiles_alone(tmp_path):
	src = tmp_path / 'only.cpp'
	src.write_text('#include "lctable_rules.h"\nint main() { return (int)tp_lctable::padded_rows(31) - 60; }\n')
	subprocess.run(['g++', '-std=c++17', '-Wall', '-fsyntax-only', '-I' + lc.CSRC, str(src)], check=True)


def test_cases_cover_the_list():
	"""The sizes and forms the packer's checks name are all among the cases."""
	assert {c.n_rows for c in CASES.values()} >= set(lc.N_ROWS)
	assert {c.n_targets for c in CASES.values()} == {1, 3, 2}
	assert any(c.rows is None for c in CASES.values()) and any(c.quality is None for c in CASES.values()) and any(c.pos_corr is None for c in CASES.values())
	assert any(c.stride == 0 for c in CASES.values()) and any(c.stride > c.T for c in CASES.values()) and any(c.stride == c.T for c in CASES.values())
	for name, first in (('dropped_first', 1), ('dropped_last', 0), ('dropped_middle', 0)):
		c = CASES[name]
		assert c.T == c.n_rows + 1 and c.rows[0] == first and (name != 'dropped_last' or c.rows[-1] == c.T - 2) and (name != 'dropped_middle' or c.rows[-1] == c.T - 1)


@pytest.mark.parametrize('name', list(CASES))
def test_bytes_and_sums_are_the_host_path_s(tmp_path, name):
	case = CASES[name]
	want, sums = case.expected()
	res = lc.host_pack(tmp_path, case)
	assert res[0] == 'ok', res
	assert len(res[1]) == case.capacity
	if res[1] != want:
		got, exp = np.frombuffer(res[1], dtype='uint8'), np.frombuffer(want, dtype='uint8')
		bad = np.flatnonzero(got != exp)
		pytest.fail(f'{name}: {len(bad)} bytes differ, the first at {bad[0]} (offsets {case.offsets}, unit {case.unit}): {got[bad[0]]:#x} for {exp[bad[0]]:#x}')
	assert np.array_equal(res[2], sums), (res[2], sums)


def test_the_special_values_are_in_the_cases():
	"""NaNs with payload and sign, signalling NaNs, -0.0, denormals and infinities lie in kept rows of a float64 column, and the bytes the
	host path writes for them are their own bits: the yardstick itself moves them as integers."""
	case = CASES['no_list_65']
	want, _ = case.expected()
	rows = np.frombuffer(want, dtype='uint8')[int(case.offsets[0]):int(case.offsets[0]) + 65 * lc.ROW].reshape(65, lc.ROW)
	time_bits = rows[:, 0:8].copy().view('>u8')[:, 0]
	assert set(int(b) for b in lc.F64_BITS) <= set(int(b) for b in time_bits)
	tc = rows[:, 8:12].copy().view('>u4')[:, 0]
	for bits in (0x3F800000, 0x3F800002, 0x3F800001, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00000001, 0x00000002, 0x80000000, 0x00800000, 0xFFC00000 | 0x0, 0x7FC00001):
		assert bits in set(int(b) for b in tc), hex(bits)
	cad = rows[:, 12:16].copy().view('>i4')[:, 0]
	assert -2**31 in cad and 2**31 - 1 in cad and -1 in cad


def test_max_rows_is_the_bound_of_the_word_sum():
	n, fits, next_fits = (int(v) for v in lc.drive('maxrows\n')[0].split())
	assert n == 2**32 // 24 == 178956970 and fits == 1 and next_fits == 0


def _small():
	return CASES['rows_31_x3']


REFUSALS = [
	('null_time', dict(null_mask=1), 'null pointer'),
	('null_timecorr', dict(null_mask=2), 'null pointer'),
	('null_cadenceno', dict(null_mask=4), 'null pointer'),
	('null_pixel_quality', dict(null_mask=8), 'null pointer'),
	('null_lc', dict(null_mask=16), 'null pointer'),
	('null_out', dict(null_mask=32), 'null pointer'),
	('null_datasum', dict(null_mask=64), 'null pointer'),
	('null_offsets', dict(null_mask=128), 'null pointer'),
	('null_description', dict(null_mask=256), 'null pointer'),
	('no_targets', dict(n_targets=0, offsets=[]), 'n_targets must lie in'),
	('negative_targets', dict(n_targets=-1, offsets=[]), 'n_targets must lie in'),
	('negative_rows', dict(n_rows=-1, has_rows=0), 'n_rows must lie in [0, T]'),
	('rows_above_T', dict(n_rows=32, has_rows=0), 'n_rows must lie in [0, T]'),
	('T_zero', dict(T=0, n_rows=0), 'T must lie in'),
	('rows_above_the_sum_bound', dict(T=178956971, n_rows=178956971, has_rows=0), 'kMaxRows'),
	('negative_stride', dict(strides=[-1, 0, 0, 0, 0, 0, 0]), 'stride is negative'),
	('offset_not_16', dict(offsets=[8, 4000, 8000]), 'no multiple of 16'),
	('range_leaves', dict(capacity=3 * 64 + 3 * 5760 - 16), 'leaves out_capacity'),
	('offset_behind_the_end', dict(offsets=[1 << 40, 64, 6000]), 'leaves out_capacity'),
	('ranges_overlap', dict(offsets=[64, 64 + 5760 - 16, 64 + 2 * 5760 + 64]), 'overlap'),
	('same_range_twice', dict(offsets=[64, 64, 64 + 5760 + 64]), 'overlap'),
	('misaligned_out', dict(misalign_mask=32), 'd_out must be 16-byte aligned'),
	('misaligned_datasum', dict(misalign_mask=64), 'd_datasum must be 8-byte aligned'),
	('misaligned_rows', dict(misalign_mask=512), 'd_rows must be 4-byte aligned'),
]


@pytest.mark.parametrize('name,how,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(tmp_path, name, how, message):
	case = _small()
	assert case.unit == 5760 and case.capacity == 4 * 64 + 3 * 5760
	res = lc.host_pack(tmp_path, case, **how)
	assert res[0] == 'refused' and message in res[1], res


def test_the_smallest_capacity_and_the_largest_row_count_are_taken(tmp_path):
	case = _small()
	tight = lc.host_pack(tmp_path, case, capacity=case.capacity - lc.GUARD)               # the last range ends with the buffer
	assert tight[0] == 'ok' and tight[1] == case.expected()[0][:case.capacity - lc.GUARD]
	touching = lc.host_pack(tmp_path, case, offsets=[0, 5760, 2 * 5760], capacity=3 * 5760)   # ranges that touch do not overlap
	want = case.expected()[0]
	assert touching[0] == 'ok' and touching[1] == b''.join(want[int(o):int(o) + 5760] for o in case.offsets)
	# n_rows == 0: ranges are empty, offsets may coincide and lie at the very end
	empty = CASES['rows_0_x3']
	res = lc.host_pack(tmp_path, empty, offsets=[empty.capacity, empty.capacity, 0])
	assert res[0] == 'ok' and res[1] == b'\xa5' * empty.capacity and not res[2].any()


PLACE = lc.place_cases()


@pytest.mark.parametrize('name', list(PLACE))
def test_place(tmp_path, name):
	src, capacity, segments = PLACE[name]
	res = lc.host_place(tmp_path, src, capacity, segments)
	assert res[0] == 'ok' and res[1] == lc.place_expected(src, capacity, segments)


PLACE_REFUSALS = [
	('null_src', dict(null_mask=1), 'null pointer'),
	('null_dst', dict(null_mask=2), 'null pointer'),
	('null_arrays', dict(null_mask=4), 'null pointer'),
	('misaligned_src', dict(misalign_mask=1), '16-byte aligned'),
	('misaligned_dst', dict(misalign_mask=2), '16-byte aligned'),
	('no_segments', dict(segments=[]), 'n_segments must lie in'),
	('src_offset_not_16', dict(segments=[(8, 0, 16)]), 'multiples of 16'),
	('dst_offset_not_16', dict(segments=[(0, 8, 16)]), 'multiples of 16'),
	('length_not_16', dict(segments=[(0, 0, 24)]), 'multiples of 16'),
	('leaves_the_source', dict(segments=[(2880, 0, 2880 + 16)]), 'leaves the source buffer'),
	('leaves_the_destination', dict(segments=[(0, 5760 - 2880 + 16, 2880)]), 'leaves the destination buffer'),
	('destinations_overlap', dict(segments=[(0, 0, 2880), (2880, 2880 - 16, 2880)]), 'overlap'),
]


@pytest.mark.parametrize('name,how,message', PLACE_REFUSALS, ids=[r[0] for r in PLACE_REFUSALS])
def test_place_refusals(tmp_path, name, how, message):
	how = dict(how)
	segments = how.pop('segments', [(0, 0, 2880), (2880, 2880, 2880)])
	res = lc.host_place(tmp_path, bytes(5760), 5760, segments, **how)
	assert res[0] == 'refused' and message in res[1], res
	ok = lc.host_place(tmp_path, bytes(5760), 5760, [(0, 2880, 2880), (2880, 0, 2880)])
	assert ok[0] == 'ok' and ok[1] == bytes(5760)
