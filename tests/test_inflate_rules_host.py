# -*- coding: utf-8 -*-
"""
CPU checks of the DEFLATE decoder's device-free rules (photometry_amd/csrc/inflate_rules.h): tests/hostsim/inflate_rules_host.cpp,
built with AddressSanitizer and UBSan, runs the rules' ``inflate_stream`` on every stream of a call, the pieces the lanes share lane
after lane, with every input and every slot a heap block of its own that ends where it ends.  Python's zlib is the yardstick
(``zlib.decompressobj(-15)``, ``.eof``, ``.unused_data``, ``zlib.crc32``): the status is ``OK`` exactly when zlib reaches the end of the
stream, and then bytes, consumed count and CRC are zlib's.  The cases (tests/inflate_common.py) are the smallest at which each rule
can go wrong; all of them, corrupt ones included, are the streams of one call, at unaligned offsets.
"""
import subprocess
import numpy as np
import pytest
import inflate_common as ic


@pytest.fixture(scope='module')
def call(tmp_path_factory):
	"""All cases as the streams of one call."""
	tmp = tmp_path_factory.mktemp('inflate')
	cases = ic.cases(tmp)
	res = ic.host_inflate(tmp, [s for s, _ in cases.values()], [n for _, n in cases.values()])
	assert res[0] == 'ok'
	return cases, res


def _at(cases, name):
	return list(cases).index(name)


def test_header_compiles_alone(tmp_path):
	src = tmp_path / 'only.cpp'
	src.write_text('#include "inflate_rules.h"\nint main() { return (int)tp_inflate_rules::length_base(257) - 3; }\n')
	subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only', '-I' + ic.CSRC, str(src)], check=True)


def test_bases_and_state_size():
	lines = ic.drive('bases\nlds\n')
	assert [int(v) for v in lines[0].split()] == ic.LENGTH_BASE
	assert [int(v) for v in lines[1].split()] == ic.DISTANCE_BASE
	assert int(lines[2]) <= 40 * 1024                                                       # four wavefronts per CU of 160 KiB


def test_ok_exactly_when_zlib_reaches_the_end(call, capsys):
	cases, (_, outputs, statuses, produced, consumed, crcs) = call
	taken, refused = ic.check_against_zlib(cases, outputs, statuses, produced, consumed, crcs)
	flips = [k for k, name in enumerate(cases) if name.startswith('flip_')]
	flips_taken = sum(1 for k in flips if statuses[k] == ic.OK)
	with capsys.disabled():
		print(f'\ninflate rules: {len(cases)} streams, {taken} taken to the end, {refused} refused; of {len(flips)} flipped bits {flips_taken} taken; '
			f'statuses {dict(zip(*np.unique(statuses, return_counts=True)))}')
	# the set exercises both answers, and every status occurs
	assert flips_taken > 1000 and len(flips) - flips_taken > 300
	assert set(int(s) for s in statuses) == set(range(10))


def test_named_cases(call):
	cases, (_, outputs, statuses, produced, consumed, _crcs) = call
	want = {'empty': ic.INPUT_ENDS, 'one_byte': ic.INPUT_ENDS, 'block_type_3': ic.BAD_BLOCK_TYPE, 'len_not_nlen': ic.STORED_LENGTH, 'hlit_287': ic.TOO_MANY_SYMBOLS,
		'hdist_31': ic.TOO_MANY_SYMBOLS, 'symbol_16_first': ic.BAD_CODE_LENGTHS, 'oversubscribed': ic.BAD_CODE_LENGTHS, 'incomplete': ic.BAD_CODE_LENGTHS,
		'run_past_the_end': ic.BAD_CODE_LENGTHS, 'empty_code_length_code': ic.BAD_CODE_LENGTHS, 'no_end_of_block': ic.NO_END_OF_BLOCK,
		'fixed_first_token_a_match': ic.DISTANCE_TOO_FAR, 'one_bit_distance_code_unused_half': ic.BAD_SYMBOL, 'empty_distance_code_used': ic.BAD_SYMBOL,
		'slot_one_short': ic.OUTPUT_FULL, 'slot_one_short_stored': ic.OUTPUT_FULL, 'slot_one_short_literal': ic.OUTPUT_FULL,
		'distance_32768': ic.OK, 'wraps_level6': ic.OK, 'stored_wraps': ic.OK, 'full_flush': ic.OK, 'stored_empty_final': ic.OK, 'fibonacci_huffman_only': ic.OK,
		'runs_across_boundary': ic.OK, 'one_bit_distance_code': ic.OK, 'text_huffman_only': ic.OK, 'rle_long_run': ic.OK, 'own_encoder': ic.OK,
		'own_encoder_stored_chunks': ic.OK, 'ends_on_a_byte': ic.OK, 'ends_inside_a_byte': ic.OK, 'slot_larger': ic.OK}
	for name, status in want.items():
		assert statuses[_at(cases, name)] == status, (name, statuses[_at(cases, name)])
	k = _at(cases, 'trailing_8')
	assert statuses[k] == ic.OK and int(consumed[k]) == len(cases['trailing_8'][0]) - 8      # the count stops at the final block's end
	k = _at(cases, 'slot_one_short_literal')
	assert outputs[k] == b'AB'                                                               # what fits is there
	assert int(produced[_at(cases, 'wraps_level6')]) == 300000


def test_every_prefix_is_refused_for_lack_of_input(call):
	cases, (_, _outputs, statuses, _produced, _consumed, _crcs) = call
	seen = 0
	for k, name in enumerate(cases):
		if name.startswith('prefix_'):
			assert statuses[k] == ic.INPUT_ENDS, (name, statuses[k])
			seen += 1
	assert seen > 100


def test_another_order_and_other_offsets_give_the_same_results(call, tmp_path):
	cases, (_, outputs, statuses, produced, consumed, crcs) = call
	names = [n for n in cases if not n.startswith('flip_') or n.endswith('0')][::-1]
	idx = [_at(cases, n) for n in names]
	res = ic.host_inflate(tmp_path, [b'x'] + [cases[n][0] for n in names], [3] + [cases[n][1] for n in names])
	assert res[0] == 'ok'
	assert res[1][1:] == [outputs[k] for k in idx]
	for got, want in zip(res[2:], (statuses, produced, consumed, crcs)):
		assert np.array_equal(got[1:], want[idx])


REFUSALS = [
	('n_streams', dict(n_streams=0, in_offsets=[0], out_offsets=[0]), 'n_streams must be at least 1'),
	('n_streams_negative', dict(n_streams=-1, in_offsets=[0], out_offsets=[0]), 'n_streams must be at least 1'),
	('null_in_offsets', dict(null_mask=64), 'null pointer'),
	('null_out_offsets', dict(null_mask=128), 'null pointer'),
	('falling_in_offsets', dict(in_offsets=[0, 2, 1, 4]), 'must not fall'),
	('falling_out_offsets', dict(out_offsets=[0, 20, 10, 40]), 'must not fall'),
	('total_in', dict(in_offsets=[0, 1 << 34], out_offsets=[0, 8], n_streams=1), 'fewer than 2^34 bytes'),
	('total_out', dict(in_offsets=[0, 2], out_offsets=[0, 1 << 34], n_streams=1), 'fewer than 2^34 bytes'),
	('null_in', dict(null_mask=1), 'null pointer'),
	('null_out', dict(null_mask=2), 'null pointer'),
	('null_status', dict(null_mask=4), 'null pointer'),
	('null_out_bytes', dict(null_mask=8), 'null pointer'),
	('null_in_bytes', dict(null_mask=16), 'null pointer'),
	('null_crc', dict(null_mask=32), 'null pointer'),
	('misaligned_status', dict(misalign_mask=4), 'd_status must be 4-byte aligned'),
	('misaligned_out_bytes', dict(misalign_mask=8), 'd_out_bytes must be 8-byte aligned'),
	('misaligned_in_bytes', dict(misalign_mask=16), 'd_in_bytes must be 8-byte aligned'),
	('misaligned_crc', dict(misalign_mask=32), 'd_crc must be 4-byte aligned'),
]


@pytest.mark.parametrize('name,how,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(tmp_path, name, how, message):
	streams, slots = [b'\x03\x00', b'', b'\x03\x00'], [10, 10, 10]
	res = ic.host_inflate(tmp_path, streams, slots, **how)
	assert res[0] == 'refused' and message in res[1], res


def test_no_bytes_need_no_data_pointer(tmp_path):
	res = ic.host_inflate(tmp_path, [b'', b''], [0, 0], null_mask=1 | 2)
	assert res[0] == 'ok' and list(res[2]) == [ic.INPUT_ENDS] * 2 and list(res[3]) == [0, 0]
