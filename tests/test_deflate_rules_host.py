# -*- coding: utf-8 -*-
"""
CPU checks of the DEFLATE encoder's device-free rules (photometry_amd/csrc/deflate_rules.h): tests/hostsim/deflate_rules_host.cpp,
built with AddressSanitizer and UBSan, composes them serially -- every chunk, every lane -- into the bytes the kernel writes, with
input, output and work buffers of exactly the size a call may touch; zlib inflates every stream (``zlib.decompressobj(-15)``) and
gives the CRCs.  The cases (tests/deflate_common.py) are the smallest inputs at which each rule can go wrong.
"""
import subprocess
import zlib
import numpy as np
import pytest
import deflate_common as dc

C = dc.C


@pytest.fixture(scope='module')
def call(tmp_path_factory):
	"""All cases as the streams of one call."""
	cases = dc.cases()
	res = dc.host_deflate(tmp_path_factory.mktemp('deflate'), list(cases.values()))
	assert res[0] == 'ok'
	return cases, res


def _chunk_range(cases, name):
	first = sum(len(dc.chunks_of(b)) for k, b in list(cases.items())[:list(cases).index(name)])
	return first, first + len(dc.chunks_of(cases[name]))


def test_header_compiles_alone(tmp_path):
	src = tmp_path / 'only.cpp'
	src.write_text('#include "deflate_rules.h"\nint main() { return (int)tp_deflate_rules::bound_of(1) - 6; }\n')
	subprocess.run(['g++', '-std=c++17', '-Wall', '-fsyntax-only', '-I' + dc.CSRC, str(src)], check=True)


def test_chunk_and_bound():
	lines = dc.drive('chunk\n' + ''.join(f'bound {n}\n' for n in (0, 1, C, C + 1, 5 * C)))
	assert [int(v) for v in lines] == [C, 0, 6, C + 5, C + 1 + 10, 5 * C + 25]
	assert C in (16384, 32768)


def test_every_stream_inflates_to_its_input(call):
	cases, (_, packed, ends, crcs, forms, _lens) = call
	dc.check_streams(list(cases.values()), packed, ends, crcs)


def test_forms(call):
	cases, (_, _packed, _ends, _crcs, forms, _lens) = call
	for name in cases:
		a, b = _chunk_range(cases, name)
		if name.startswith('random_') or name == 'all_values':
			assert all(f == dc.STORED for f in forms[a:b]), name                         # incompressible: the stored form
	# all three forms occur
	assert set(forms) == {dc.STORED, dc.FIXED, dc.DYNAMIC}
	a, b = _chunk_range(cases, f'zeros_{C}')
	assert forms[a:b] == [dc.DYNAMIC]


def test_far_matches_are_found(call):
	cases, (_, _packed, ends, _crcs, _forms, _lens) = call
	for name in ('far', 'far_end'):
		a, b = _chunk_range(cases, name)
		size = int(ends[a]) - (int(ends[a - 1]) if a else 0)
		assert b == a + 1 and size < C // 2 + 400, (name, size)                           # the second half costs a few hundred bytes at the most


def test_no_match_across_the_chunk_boundary(call, tmp_path):
	cases, (_, packed, ends, _crcs, _forms, _lens) = call
	a, b = _chunk_range(cases, 'boundary')
	assert b == a + 2
	blob = cases['boundary']
	for c, piece in ((a, blob[:C]), (a + 1, blob[C:])):                                    # each chunk inflates alone
		d = zlib.decompressobj(-15)
		assert d.decompress(packed[int(ends[c - 1]) if c else 0:int(ends[c])] + b'\x03\x00') == piece and d.eof
	# the same second chunk as a stream of its own gives the same bytes: nothing of chunk 0 went into it
	alone = dc.host_deflate(tmp_path, [blob[C:]])
	assert alone[1] == packed[int(ends[a]):int(ends[a + 1])]


def _kraft(lengths):
	return sum(2.0 ** -l for l in lengths if l)


def test_code_builder_on_counts():
	fib = dc.fibonacci(22)                                                                 # an unlimited Huffman code is 21 bits deep
	jobs = [(fib, 15), (fib[::-1], 15), (fib[:9], 15), (fib[:12], 7), ([5, 0, 0, 9], 15), ([0, 0, 7], 15), ([7, 0, 0], 15), ([0] * 30, 15), ([1] * 286, 15), ([1] * 19, 7),
		(list(range(1, 287)), 15), ([1] * 285 + [10 ** 6], 15)]
	lines = dc.drive(''.join(f"codes {len(f)} {m} {' '.join(map(str, f))}\n" for f, m in jobs))
	for (freq, most), line in zip(jobs, lines):
		lens = [int(v) for v in line.split()[1:]]
		used = [l for l, f in zip(lens, freq) if f]
		assert len(lens) == len(freq) and all(l > 0 for l in used) and max(lens) <= most
		if len(used) >= 2:
			assert _kraft(lens) == 1.0 and all(l == 0 for l, f in zip(lens, freq) if not f)
			# a rarer symbol never has the shorter code
			order = sorted(range(len(freq)), key=lambda s: freq[s])
			assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:]) if freq[a] and freq[a] < freq[b])
		elif len(used) == 1:
			assert sorted(l for l in lens if l) == [1, 1]                                   # the used symbol and a second one: a complete code
		else:
			assert not any(lens)
	lens = [int(v) for v in lines[0].split()[1:]]
	assert max(lens) == 15                                                                 # the limiter acted
	# optimal where no limit binds: the weighted length of Huffman's code
	lens = [int(v) for v in lines[2].split()[1:]]                                          # (job 2: nine symbols, 8 bits deep)
	assert sum(l * f for l, f in zip(lens, fib[:9])) == sum(l * f for l, f in zip([8, 8, 7, 6, 5, 4, 3, 2, 1], fib[:9]))


def test_code_builder_in_chunks(call):
	cases, (_, _packed, _ends, _crcs, forms, lens) = call
	seen = 0
	for c, ll in enumerate(lens):
		if ll is None:
			continue
		seen += 1
		assert forms[c] == dc.DYNAMIC and len(ll) == 286 and max(ll) <= 15 and ll[256] > 0 and _kraft(ll) == 1.0, c
	assert seen >= 10
	for name in ('one_value', 'two_values', 'fibonacci', 'header_runs', f'zeros_{C}'):
		a, b = _chunk_range(cases, name)
		assert forms[a] in (dc.DYNAMIC, dc.FIXED), name


def test_header_coding_case_has_the_runs_it_is_made_for(call):
	cases, (_, _packed, _ends, _crcs, forms, lens) = call
	a, _b = _chunk_range(cases, 'header_runs')
	ll = lens[a]
	assert forms[a] == dc.DYNAMIC
	assert all(l == 0 for l in ll[101:240]) and ll[100] > 0 and ll[240] > 0                 # 138 + 1 zero lengths: symbol 18 is split
	assert len(set(ll[1:8])) == 1 and ll[0] != ll[1] and ll[8] != ll[1]                     # 6 + 1 equal lengths: symbol 16 behind its literal


def test_crc_combine(call):
	cases, (_, _packed, _ends, crcs, _forms, _lens) = call
	name = f'random_{2 * C + 5}'
	a, b = _chunk_range(cases, name)
	pieces = dc.chunks_of(cases[name])
	text, want = '', []
	run = 0
	for k, piece in enumerate(pieces):                                                     # fold over the chunks
		text += f'combine {run} {int(crcs[a + k])} {len(piece)}\n'
		run = zlib.crc32(piece, run)
		want.append(run)
	assert run == zlib.crc32(cases[name])
	blob = cases[name][:300]
	for la, lb in ((300, 0), (299, 1), (0, 300), (1, 299), (0, 0), (7, 293)):
		text += f'combine {zlib.crc32(blob[:la])} {zlib.crc32(blob[la:la + lb])} {lb}\n'
		want.append(zlib.crc32(blob[:la + lb]))
	text += f'combine {zlib.crc32(b"abc")} {zlib.crc32(bytes(1 << 20))} {1 << 20}\n'
	want.append(zlib.crc32(b'abc' + bytes(1 << 20)))
	assert [int(v) for v in dc.drive(text)] == want


def test_two_runs_and_another_stream_order_give_the_same_bytes(call, tmp_path):
	cases, (_, packed, ends, crcs, _forms, _lens) = call
	names = list(cases)[::-1]
	res = dc.host_deflate(tmp_path, [cases[n] for n in names])
	dc.check_streams([cases[n] for n in names], res[1], res[2], res[3])
	# a stream's bytes do not depend on its place in the call
	at = {}
	c, begin = 0, 0
	for n in cases:
		k = len(dc.chunks_of(cases[n]))
		end = int(ends[c + k - 1]) if k else begin
		at[n] = packed[begin:end]
		c, begin = c + k, end
	c, begin = 0, 0
	for n in names:
		k = len(dc.chunks_of(cases[n]))
		end = int(res[2][c + k - 1]) if k else begin
		assert res[1][begin:end] == at[n], n
		c, begin = c + k, end
	# an unaligned first stream: every stream behind it begins at another address modulo 4
	again = dc.host_deflate(tmp_path, [b'x'] + list(cases.values()))
	assert again[1][6:] == packed and np.array_equal(again[2][1:], ends + 6)


REFUSALS = [
	('n_streams', dict(n_streams=0, offsets=[0]), 'n_streams must be at least 1'),
	('n_streams_negative', dict(n_streams=-1, offsets=[0]), 'n_streams must be at least 1'),
	('null_offsets', dict(null_mask=32), 'null pointer'),
	('falling_offsets', dict(offsets=[0, 50, 40, 100]), 'must not fall'),
	('total', dict(offsets=[0, 1 << 34], n_streams=1), 'fewer than 2^34 bytes'),
	('null_in', dict(null_mask=1), 'null pointer'),
	('null_out', dict(null_mask=2), 'null pointer'),
	('null_end', dict(null_mask=4), 'null pointer'),
	('null_crc', dict(null_mask=8), 'null pointer'),
	('null_work', dict(null_mask=16), 'null pointer'),
	('misaligned_end', dict(misalign_mask=4), 'd_chunk_end must be 8-byte aligned'),
	('misaligned_crc', dict(misalign_mask=8), 'd_chunk_crc must be 4-byte aligned'),
	('misaligned_work', dict(misalign_mask=16), 'd_work must be 16-byte aligned'),
	('capacity', dict(out_capacity=50 + 5 + 50 + 5 - 1), 'out_capacity is below'),
	('work', dict(work_bytes='short'), 'work buffer is smaller'),
]


@pytest.mark.parametrize('name,how,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(tmp_path, name, how, message):
	blobs = [bytes(50), b'', bytes(range(50))]
	how = dict(how)
	if how.get('work_bytes') == 'short':
		how['work_bytes'] = 2 * (16 + 4 * C + 16400) + 16 - 1
	res = dc.host_deflate(tmp_path, blobs, **how)
	assert res[0] == 'refused' and message in res[1], res
	ok = dc.host_deflate(tmp_path, blobs, out_capacity=110, work_bytes=2 * (16 + 4 * C + 16400) + 16)
	assert ok[0] == 'ok'                                                                   # the smallest sizes that are taken


def test_no_input_needs_no_pointer(tmp_path):
	res = dc.host_deflate(tmp_path, [b'', b''], null_mask=1 | 2 | 4 | 8 | 16)
	assert res[0] == 'ok' and res[1] == b'' and len(res[2]) == 0


def test_size_on_a_light_curve_table(tmp_path, capsys):
	"""Keeps a stored-only or a fixed-only encoder from passing: on the first 600 000 bytes of a 19 000-row light-curve file the output
	is smaller than zlib's Z_FIXED level-1 raw deflate of the same bytes.  The ratios to zlib's levels are printed: measurements."""
	blob = dc.lightcurve_table()
	res = dc.host_deflate(tmp_path, [blob])
	dc.check_streams([blob], res[1], res[2], res[3])
	size = len(res[1]) + 2
	fixed = len(dc.zlib_raw(blob, 1, zlib.Z_FIXED))
	huffman = len(dc.zlib_raw(blob, 1, zlib.Z_HUFFMAN_ONLY))
	levels = {level: len(dc.zlib_raw(blob, level)) for level in (1, 6, 9)}
	with capsys.disabled():
		print(f'\ndeflate rules on {len(blob)} bytes of a light-curve file: {size} bytes; Z_FIXED {fixed}, Z_HUFFMAN_ONLY {huffman}; '
			+ ', '.join(f'level {k}: {v} (ratio {size / v:.4f})' for k, v in levels.items()) + f'; forms {sorted(set(res[4]))}')
	assert size < fixed
	# random bytes: never above the bound
	noise = np.random.default_rng(5).integers(0, 256, 3 * C + 77, dtype='uint8').tobytes()
	res = dc.host_deflate(tmp_path, [noise], name='noise')
	assert len(res[1]) <= len(noise) + 5 * 4 and all(f == dc.STORED for f in res[4])
