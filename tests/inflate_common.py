# -*- coding: utf-8 -*-
"""
What the tests of the DEFLATE decoder share (tests/test_inflate_rules_host.py, tests/test_gpu_inflate.py): the case streams -- the
smallest at which each rule of photometry_amd/csrc/inflate_rules.h can go wrong, corrupt ones included --, a bit writer for the
hand-built ones, the host driver tests/hostsim/inflate_rules_host.cpp built with AddressSanitizer and UBSan, and zlib's verdict on a
stream (``zlib.decompressobj(-15)``): the yardstick.
"""
import os
import subprocess
import zlib
import numpy as np
import conftest
import deflate_common as dc

CSRC = dc.CSRC
SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'inflate_rules_host.cpp')
OUT = os.path.join(dc.OUT_DIR, 'inflate_rules_host')
WINDOW = 32768
OK, INPUT_ENDS, BAD_BLOCK_TYPE, STORED_LENGTH, TOO_MANY_SYMBOLS, BAD_CODE_LENGTHS, NO_END_OF_BLOCK, BAD_SYMBOL, DISTANCE_TOO_FAR, OUTPUT_FULL = range(10)
SENTINEL = 0xC7
#: slot of a stream that zlib does not take to its end
REFUSED_SLOT = 4096

# RFC 1951, 3.2.5
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DISTANCE_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DISTANCE_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
#: a complete code-length code over all 19 symbols: 13 of 4 bits, 6 of 5 bits
CL_LENS = [4] * 13 + [5] * 6


def build_driver():
	"""The driver, compiled once per run of the suite (``-fno-sanitize-recover``: a report ends the program)."""
	os.makedirs(dc.OUT_DIR, exist_ok=True)
	deps = [SRC] + [os.path.join(CSRC, h) for h in ('inflate_rules.h', 'deflate_rules.h', 'fits_rules.h')]
	if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
		subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-I' + CSRC, SRC, '-o', OUT], check=True)
	return OUT


def drive(text):
	r = subprocess.run([build_driver()], input=text, capture_output=True, text=True)
	assert r.returncode == 0 and 'FAILED' not in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
	return r.stdout.splitlines()


def offsets_of(sizes):
	return np.concatenate([[0], np.cumsum(sizes)]).astype('uint64')


def host_inflate(tmp, streams, slots, null_mask=0, misalign_mask=0, n_streams=None, in_offsets=None, out_offsets=None, name='call'):
	"""One ``inflate`` command: ``('ok', outputs, statuses, produced, consumed, crcs)`` -- outputs a list of ``bytes``, the rest arrays --
	or ``('refused', message)``; the output file must be absent after a refusal."""
	inp, out = os.path.join(str(tmp), name + '.in'), os.path.join(str(tmp), name + '.out')
	with open(inp, 'wb') as fh:
		fh.write(b''.join(streams))
	if os.path.exists(out):
		os.remove(out)
	in_offsets = offsets_of([len(s) for s in streams]) if in_offsets is None else in_offsets
	out_offsets = offsets_of(slots) if out_offsets is None else out_offsets
	n_streams = len(streams) if n_streams is None else n_streams
	lines = drive(f"inflate {inp} {out} {n_streams} {' '.join(str(int(o)) for o in in_offsets)} {' '.join(str(int(o)) for o in out_offsets)} {null_mask} {misalign_mask}\n")
	if lines[0].startswith('refused '):
		assert not os.path.exists(out)
		return 'refused', lines[0][len('refused '):]
	assert lines[0] == f'ok streams {n_streams}', lines[0]
	rows = np.array([[int(v) for v in line.split()[1:]] for line in lines[1:]], dtype='int64').reshape(-1, 4)
	assert len(rows) == n_streams and all(line.startswith('stream ') for line in lines[1:])
	with open(out, 'rb') as fh:
		packed = fh.read()
	ends = np.cumsum(rows[:, 1])
	assert len(packed) == (int(ends[-1]) if n_streams else 0)
	outputs = [packed[int(e) - int(n):int(e)] for e, n in zip(ends, rows[:, 1])]
	return 'ok', outputs, rows[:, 0].astype('int32'), rows[:, 1].astype('uint64'), rows[:, 2].astype('uint64'), rows[:, 3].astype('uint32')


def zlib_verdict(stream):
	"""``(bytes, consumed, crc)`` when zlib takes the raw deflate stream to its end, else None."""
	d = zlib.decompressobj(-15)
	try:
		out = d.decompress(stream)
	except zlib.error:
		return None
	if not d.eof:
		return None
	return out, len(stream) - len(d.unused_data), zlib.crc32(out)


# ---- a bit writer for the hand-built streams ------------------------------------------------------------------------------------------
class Bits:
	def __init__(self):
		self.acc, self.n = 0, 0

	def put(self, value, nbits):
		"""``nbits`` of ``value``, least significant first."""
		self.acc |= (value & ((1 << nbits) - 1)) << self.n
		self.n += nbits

	def code(self, code_and_length):
		"""A Huffman code: most significant bit first."""
		code, length = code_and_length
		self.put(int(format(code, f'0{length}b')[::-1], 2) if length else 0, length)

	def align(self):
		self.n = (self.n + 7) & ~7

	def bytes(self):
		return self.acc.to_bytes((self.n + 7) // 8, 'little')


def codes_of(lens):
	"""Canonical codes (RFC 1951, 3.2.2): symbol -> (code, length)."""
	count = [0] * 17
	for l in lens:
		count[l] += 1
	count[0] = 0
	code, nxt = 0, [0] * 17
	for b in range(1, 17):
		code = (code + count[b - 1]) << 1
		nxt[b] = code
	out = {}
	for s, l in enumerate(lens):
		if l:
			out[s] = (nxt[l], l)
			nxt[l] += 1
	return out


def put_tokens(w, tokens, ll, d):
	"""Literals (ints) and matches (``(length, distance)``) under the codes ``ll`` and ``d``; ``'eob'`` ends the block."""
	for t in tokens:
		if t == 'eob':
			w.code(ll[256])
		elif isinstance(t, tuple):
			length, dist = t
			ls = max(s for s in range(29) if LENGTH_BASE[s] <= length) if length < 258 else 28
			w.code(ll[257 + ls])
			w.put(length - LENGTH_BASE[ls], LENGTH_EXTRA[ls])
			ds = max(s for s in range(30) if DISTANCE_BASE[s] <= dist)
			w.code(d[ds])
			w.put(dist - DISTANCE_BASE[ds], DISTANCE_EXTRA[ds])
		else:
			w.code(ll[t])


def put_stored(w, final, blob):
	w.put(final, 1)
	w.put(0, 2)
	w.align()
	w.put(len(blob), 16)
	w.put(len(blob) ^ 0xFFFF, 16)
	for b in blob:
		w.put(b, 8)


def put_fixed(w, final, tokens):
	w.put(final, 1)
	w.put(1, 2)
	put_tokens(w, tokens, codes_of(FIXED_LL), codes_of(FIXED_D))


def put_dynamic_header(w, final, hlit, hdist, items, cl_lens=CL_LENS):
	"""A dynamic block's header: ``items`` are the code-length symbols as ints (0 .. 15) or ``(16 | 17 | 18, extra)``."""
	w.put(final, 1)
	w.put(2, 2)
	w.put(hlit - 257, 5)
	w.put(hdist - 1, 5)
	w.put(19 - 4, 4)
	for s in CL_ORDER:
		w.put(cl_lens[s], 3)
	cl = codes_of(cl_lens)
	for it in items:
		if isinstance(it, tuple):
			w.code(cl[it[0]])
			w.put(it[1], {16: 2, 17: 3, 18: 7}[it[0]])
		else:
			w.code(cl[it])


def put_dynamic(w, final, ll_lens, d_lens, tokens, items=None):
	put_dynamic_header(w, final, len(ll_lens), len(d_lens), list(ll_lens) + list(d_lens) if items is None else items)
	put_tokens(w, tokens, codes_of(ll_lens), codes_of(d_lens))


#: a complete literal/length code of 258 symbols: the literals 0 .. 223 in 8 bits, 224 .. 255 unused, end-of-block and length 3 in 4 bits
RUN_LL = [8] * 224 + [0] * 32 + [4, 4]


def built(fn):
	w = Bits()
	fn(w)
	return w.bytes()


def raw(blob, level, strategy=zlib.Z_DEFAULT_STRATEGY):
	return dc.zlib_raw(blob, level, strategy)


def words(rng, n):
	"""About ``n`` bytes of text from 200 random words: compressible, with matches at all distances."""
	vocabulary = [bytes(rng.integers(97, 123, rng.integers(2, 10), dtype='uint8')) for _ in range(200)]
	out, size = [], 0
	while size < n:
		out.append(vocabulary[int(rng.integers(0, 200))])
		size += len(out[-1]) + 1
	return b' '.join(out)[:n]


def strategies(blob):
	"""name -> raw deflate stream of ``blob`` under each of zlib's levels and strategies the cases use."""
	return {'level0': raw(blob, 0), 'level1': raw(blob, 1), 'level6': raw(blob, 6), 'level9': raw(blob, 9), 'fixed': raw(blob, 6, zlib.Z_FIXED),
		'huffman_only': raw(blob, 6, zlib.Z_HUFFMAN_ONLY), 'rle': raw(blob, 6, zlib.Z_RLE)}


def cases(tmp):
	"""name -> (stream, slot bytes), in a fixed order.  The slot of a stream that zlib takes to its end is exactly its content unless
	the name says otherwise; ``tmp``: a directory for the host encoder's files."""
	rng = np.random.default_rng(21)
	rand = lambda n: rng.integers(0, 256, n, dtype='uint8').tobytes() # noqa: E731
	out = {}

	def add(name, stream, slot=None):
		v = zlib_verdict(stream)
		out[name] = (stream, (len(v[0]) if v else REFUSED_SLOT) if slot is None else slot)
	add('empty', b'')
	add('one_byte', b'\x03')
	text = words(rng, 20000)
	for name, stream in strategies(text).items():
		add(f'text_{name}', stream)
	add('rle_long_run', raw(b'ab' + b'\x55' * 5000 + b'cd', 6, zlib.Z_RLE))                  # distance 1, length 258
	# window: a match of 258 bytes at distance exactly 32768 whose source and whose target straddle the ring's wrap; the bytes around
	# it are stored blocks of 65535 bytes and less that cross the wrap as well
	block, body = rand(300), rand(2 * WINDOW + 1000)
	content = body[:WINDOW - 150] + block + body[WINDOW + 150:]

	def far(w):
		at = 0
		while at < 2 * WINDOW - 150:
			n = min(65535, 2 * WINDOW - 150 - at)
			put_stored(w, 0, content[at:at + n])
			at += n
		put_fixed(w, 0, [(258, WINDOW), (42, WINDOW), 'eob'])
		put_stored(w, 1, content[2 * WINDOW + 150:])
	add('distance_32768', built(far))
	assert zlib_verdict(out['distance_32768'][0])[0] == content[:2 * WINDOW - 150] + block + content[2 * WINDOW + 150:]
	big = words(rng, 300000)
	add('wraps_level6', raw(big, 6))                                                         # the ring wraps nine times, matches cross the wrap
	add('stored_wraps', raw(rand(100000), 0))                                                # stored blocks of 65535 bytes across the wrap
	c = zlib.compressobj(6, zlib.DEFLATED, -15)
	add('full_flush', c.compress(text[:3000]) + c.flush(zlib.Z_FULL_FLUSH) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[3000:6000]) + c.flush())   # empty stored blocks mid-stream
	add('stored_empty_final', built(lambda w: put_stored(w, 1, b'')))
	# code tables
	fib = dc.fibonacci(19)
	skewed = rng.permutation(np.repeat(np.arange(19, dtype='uint8') * 13, fib)).tobytes()
	add('fibonacci_huffman_only', raw(skewed, 6, zlib.Z_HUFFMAN_ONLY))                       # 15-bit codes
	add('fibonacci_level9', raw(skewed, 9))
	d16 = [4] * 16
	run_items = [8, (16, 3)] * 32 + [(18, 32 - 11), 4, (16, 3), (16, 3), (16, 2)]             # 224 eights, 32 zeros, eighteen fours across the boundary at 258
	lits = [int(v) for v in rng.integers(0, 224, 40)]
	add('runs_across_boundary', built(lambda w: put_dynamic(w, 1, RUN_LL, d16, lits + [(3, 7), (3, 40)] + lits[:5] + ['eob'], items=run_items)))
	add('run_past_the_end', built(lambda w: put_dynamic(w, 1, RUN_LL, d16, lits + ['eob'], items=run_items[:-1] + [(16, 3)])))
	add('one_bit_distance_code', built(lambda w: put_dynamic(w, 1, RUN_LL, [1], lits + [(3, 1), (3, 1)] + lits[:3] + ['eob'])))
	add('one_bit_distance_code_unused_half', built(lambda w: (put_dynamic(w, 1, RUN_LL, [0, 1], lits + [(3, 2)]), w.code(codes_of(RUN_LL)[257]), w.put(1, 1), w.code(codes_of(RUN_LL)[256]))))
	add('empty_distance_code_used', built(lambda w: (put_dynamic(w, 1, RUN_LL, [0], lits), w.code(codes_of(RUN_LL)[257]), w.put(0, 8), w.code(codes_of(RUN_LL)[256]))))
	# ends
	add('ends_on_a_byte', raw(b'stored bytes', 0))
	add('ends_inside_a_byte', b'\x03\x00')
	add('trailing_8', raw(text[:500], 6) + b'TRAILER!', slot=500)
	add('slot_larger', raw(text[:700], 6), slot=800)
	add('slot_one_short', raw(text[:700], 6), slot=699)
	add('slot_one_short_stored', raw(text[:700], 0), slot=699)
	add('slot_one_short_literal', built(lambda w: put_fixed(w, 1, [65, 66, 67, 'eob'])), slot=2)
	# the project's own encoder: chunks that end in empty stored blocks, then 03 00
	own = text[:9000] + rand(700) + bytes(3000)
	res = dc.host_deflate(tmp, [own, rand(dc.C + 10)], name='own')
	first_end = int(res[2][0])
	add('own_encoder', res[1][:first_end] + b'\x03\x00')
	add('own_encoder_stored_chunks', res[1][first_end:] + b'\x03\x00')
	# hand-built corrupt streams
	add('fixed_first_token_a_match', built(lambda w: put_fixed(w, 1, [(3, 1), 'eob'])))
	add('block_type_3', b'\x07\x00\x00')
	add('len_not_nlen', b'\x01\x05\x00\x00\x00hello')
	add('hlit_287', built(lambda w: put_dynamic_header(w, 1, 287, 1, [8] * 288)))
	add('hdist_31', built(lambda w: put_dynamic_header(w, 1, 257, 31, [8] * 288)))
	add('symbol_16_first', built(lambda w: put_dynamic(w, 1, RUN_LL, d16, lits + ['eob'], items=[(16, 0)] + run_items)))
	add('oversubscribed', built(lambda w: put_dynamic_header(w, 1, 258, 1, [1, 1, 1] + [8] * 221 + [0] * 32 + [4, 4, 1])))
	add('incomplete', built(lambda w: put_dynamic_header(w, 1, 258, 1, [8] * 200 + [0] * 56 + [4, 4, 1])))
	add('no_end_of_block', built(lambda w: put_dynamic_header(w, 1, 258, 1, [8] * 224 + [0] * 32 + [0, 3, 1])))
	add('empty_code_length_code', built(lambda w: put_dynamic_header(w, 1, 257, 1, [], cl_lens=[0] * 19)) + bytes(40))
	# every prefix of three short streams
	for name, stream in (('fixed', raw(b'hello hello hello!', 6, zlib.Z_FIXED)), ('dynamic', raw(text[:150] + text[:60], 9)), ('stored', raw(b'stored bytes', 0))):
		for k in range(1, len(stream)):
			add(f'prefix_{name}_{k}', stream[:k])
	# every third bit flipped, one at a time, in a stream of about 1 KB from each strategy
	for name, stream in strategies(text[:2600]).items():
		stream = stream if name != 'level0' else raw(text[:1000], 0)
		for bit in range(0, 8 * len(stream), 3):
			flipped = bytearray(stream)
			flipped[bit >> 3] ^= 1 << (bit & 7)
			add(f'flip_{name}_{bit}', bytes(flipped))
	return out


def check_against_zlib(cases_, outputs, statuses, produced, consumed, crcs):
	"""The rule for every stream: status ``OK`` exactly when zlib reaches ``eof`` within the slot, and then bytes, consumed count and CRC
	are zlib's; returns how many streams zlib took and refused."""
	taken = refused = 0
	for k, (name, (stream, slot)) in enumerate(cases_.items()):
		v = zlib_verdict(stream)
		if v is None or len(v[0]) > slot:
			assert statuses[k] != OK, (name, statuses[k])
			assert int(produced[k]) <= slot and len(outputs[k]) == int(produced[k]), name
			if v is not None:
				assert statuses[k] == OUTPUT_FULL and outputs[k] == v[0][:len(outputs[k])], name
			refused += 1
			continue
		assert statuses[k] == OK, (name, statuses[k])
		assert outputs[k] == v[0], name
		assert int(consumed[k]) == v[1] and int(crcs[k]) == v[2], (name, consumed[k], v[1], crcs[k], v[2])
		taken += 1
	return taken, refused
