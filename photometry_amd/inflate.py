# -*- coding: utf-8 -*-
"""
gzip members inflated on the device: many compressed byte strings decoded in one launch (``tp_inflate``, csrc/inflate.hip; what the
decoder decides in csrc/inflate_rules.h and DESIGN.md section 20).  One wavefront decodes a stream, so the device pays off with
hundreds of members per call.

* :func:`inflate_streams` -- the raw form of one call: raw deflate streams (RFC 1951) into slots of given sizes; outputs, statuses,
  consumed bytes and CRCs;
* :func:`gunzip_many` -- a list of gzip members into the list of their contents;
* :func:`gunzip_to_device` -- the same, the contents left in one device array, with their offsets.

The gzip framing is host work: the header (FEXTRA, FNAME, FCOMMENT, FHCRC) is parsed here, every slot is sized from the trailer's
ISIZE, and the trailer's CRC-32 is compared with the one the device formed over the bytes it produced.  The staging goes through the
context's pooled page-locked blocks: one upload, one ``tp_inflate``, one download of the results, one of the bytes.
"""
import struct
import zlib
import numpy as np
from .device import round_up

#: names of the statuses of ``tp_inflate`` (``enum tp_inflate_status``)
STATUS_NAMES = ('OK', 'INPUT_ENDS', 'BAD_BLOCK_TYPE', 'STORED_LENGTH', 'TOO_MANY_SYMBOLS', 'BAD_CODE_LENGTHS', 'NO_END_OF_BLOCK', 'BAD_SYMBOL', 'DISTANCE_TOO_FAR', 'OUTPUT_FULL')
OK = 0
#: the most bytes (compressed plus inflated) of one ``tp_inflate`` call of :func:`gunzip_many`
MAX_BATCH_BYTES = 512 << 20
#: no deflate stream expands further: a match of 258 bytes costs at least two bits
MAX_RATIO = 1032
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


class InflateError(ValueError):
	"""A gzip member that cannot be inflated: ``index`` is its place in the call, ``status`` the name of what is wrong."""

	def __init__(self, index, status, what=None):
		self.index, self.status = index, status
		super(InflateError, self).__init__(what or f'gzip member {index}: {status}')


def status_name(status):
	status = int(status)
	return STATUS_NAMES[status] if 0 <= status < len(STATUS_NAMES) else f'status {status}'


def header_length(member, index=0):
	"""The bytes of a gzip member's header (RFC 1952), from the member or from its front: where the raw deflate stream begins.  Raises
	:class:`InflateError` (status ``'FRAMING'``) for a header that is none or does not end in what is given."""
	n = len(member)

	def bad(what):
		return InflateError(index, 'FRAMING', f'gzip member {index}: {what}')
	if n < 10:
		raise bad('shorter than a header')
	if member[0] != 0x1F or member[1] != 0x8B or member[2] != 8:
		raise bad('not a gzip member with the deflate method')
	flags = member[3]
	if flags & 0xE0:
		raise bad('reserved flag bits set')
	at = 10
	if flags & FEXTRA:
		if at + 2 > n:
			raise bad('the header leaves the member')
		at += 2 + struct.unpack_from('<H', member, at)[0]
	for flag in (FNAME, FCOMMENT):
		if flags & flag:
			end = bytes(member[at:n]).find(b'\x00') if at < n else -1
			if end < 0:
				raise bad('the header leaves the member')
			at += end + 1
	if flags & FHCRC:
		if at + 2 > n or struct.unpack_from('<H', member, at)[0] != (zlib.crc32(bytes(member[:at])) & 0xFFFF):
			raise bad('wrong header CRC')
		at += 2
	if at > n:
		raise bad('the header leaves the member')
	return at


def parse_member(member, index=0):
	"""The framing of one gzip member: ``(begin, end, crc, isize)`` -- the raw deflate stream is ``member[begin:end]``, the trailer's
	CRC-32 and ISIZE follow it.  Raises :class:`InflateError` (status ``'FRAMING'``) for anything else."""
	n = len(member)
	if n < 18:
		raise InflateError(index, 'FRAMING', f'gzip member {index}: shorter than a header and a trailer')
	at = header_length(member, index)
	if at > n - 8:
		raise InflateError(index, 'FRAMING', f'gzip member {index}: the header leaves the member')
	crc, isize = struct.unpack_from('<II', member, n - 8)
	return at, n - 8, crc, isize


class _Call(object):
	"""One ``tp_inflate`` over ``streams`` (bytes-like) into slots of ``sizes`` bytes: the device arrays and the downloaded results."""

	def __init__(self, ctx, streams, sizes):
		self.ctx = ctx
		lib = ctx.lib
		n = self.n = len(streams)
		self.in_offsets = np.zeros(n + 1, dtype='uint64')
		self.in_offsets[1:] = np.cumsum([len(s) for s in streams], dtype='uint64')
		self.out_offsets = np.zeros(n + 1, dtype='uint64')
		self.out_offsets[1:] = np.cumsum([int(s) for s in sizes], dtype='uint64')
		total_in, self.total_out = int(self.in_offsets[-1]), int(self.out_offsets[-1])
		words = max(round_up(total_in, 4) // 4, 1)
		self.d_in = self.d_out = self.d_meta = None
		up = ctx.pinned_block(4 * words)
		meta = ctx.pinned_block(24 * n)
		try:
			at = 0
			for s in streams:
				up.array[at:at + len(s)] = np.frombuffer(s, dtype='uint8')
				at += len(s)
			self.d_in = ctx.empty(4 * words, 'uint8')
			self.d_out = ctx.empty(max(self.total_out, 4), 'uint8')
			self.d_meta = ctx.empty(24 * n, 'uint8')                    # produced and consumed (uint64 each), statuses (int32), CRCs (uint32)
			ctx._check(lib.tp_upload_cube_async(ctx.handle, self.d_in.ptr, words, up.ptr, words, 1, words))
			ctx._check(lib.tp_inflate(ctx.handle, self.d_in.ptr, self.in_offsets.ctypes.data, n, self.d_out.ptr, self.out_offsets.ctypes.data,
				self.d_meta.ptr + 16 * n, self.d_meta.ptr, self.d_meta.ptr + 8 * n, self.d_meta.ptr + 20 * n))
			ctx.download_async(meta, self.d_meta, nbytes=24 * n)
			ctx.sync()
			self.produced = np.array(meta.array[:8 * n].view('uint64'))
			self.consumed = np.array(meta.array[8 * n:16 * n].view('uint64'))
			self.statuses = np.array(meta.array[16 * n:20 * n].view('int32'))
			self.crcs = np.array(meta.array[20 * n:24 * n].view('uint32'))
		except BaseException:
			self.free()
			raise
		finally:
			ctx.pinned_release(meta)
			ctx.pinned_release(up)

	def outputs(self):
		"""The bytes every stream produced, as a list of ``bytes``: one download of the slots."""
		ctx = self.ctx
		if self.total_out == 0:
			return [b''] * self.n
		down = ctx.pinned_block(self.total_out)
		try:
			ctx.download_async(down, self.d_out, nbytes=self.total_out)
			ctx.sync()
			view = memoryview(down.array)
			return [bytes(view[int(o):int(o) + int(p)]) for o, p in zip(self.out_offsets[:-1], self.produced)]
		finally:
			ctx.pinned_release(down)

	def take_output(self):
		d_out, self.d_out = self.d_out, None
		return d_out

	def free(self):
		for name in ('d_in', 'd_out', 'd_meta'):
			d = getattr(self, name)
			if d is not None:
				d.free()
				setattr(self, name, None)


def inflate_streams(ctx, streams, sizes):
	"""
	One ``tp_inflate`` call over the raw deflate streams ``streams``, stream ``s`` into a slot of ``sizes[s]`` bytes:
	``(outputs, statuses, consumed, crcs)`` -- the bytes every stream produced (a list of ``bytes``), its status (int32, see
	:data:`STATUS_NAMES`), the input bytes up to the end of its final block (uint64) and the CRC-32 of what it produced (uint32).
	A stream whose status is not ``OK`` has the bytes it produced before its rule broke.
	"""
	streams = [bytes(s) for s in streams]
	if len(streams) != len(sizes):
		raise ValueError('one slot size per stream')
	if not streams:
		return [], np.zeros(0, dtype='int32'), np.zeros(0, dtype='uint64'), np.zeros(0, dtype='uint32')
	call = _Call(ctx, streams, sizes)
	try:
		return call.outputs(), call.statuses, call.consumed, call.crcs
	finally:
		call.free()


def _gunzip_call(ctx, members, first):
	"""One call over ``members`` (their place in the caller's list begins at ``first``), checked: the :class:`_Call`, device arrays alive."""
	frames = [parse_member(m, first + k) for k, m in enumerate(members)]
	for k, (begin, end, _crc, isize) in enumerate(frames):
		if isize > MAX_RATIO * (end - begin) + 16:
			raise InflateError(first + k, 'ISIZE', f'gzip member {first + k}: ISIZE {isize} is more than {end - begin} bytes of deflate can hold')
	call = _Call(ctx, [memoryview(m)[begin:end] for m, (begin, end, _c, _i) in zip(members, frames)], [isize for _b, _e, _c, isize in frames])
	try:
		for k, (begin, end, crc, isize) in enumerate(frames):
			if call.statuses[k] != OK:
				raise InflateError(first + k, status_name(call.statuses[k]))
			if int(call.produced[k]) != isize:
				raise InflateError(first + k, 'ISIZE', f'gzip member {first + k}: {int(call.produced[k])} bytes where ISIZE says {isize}')
			if int(call.crcs[k]) != crc:
				raise InflateError(first + k, 'CRC', f'gzip member {first + k}: CRC-32 {int(call.crcs[k]):08x} where the trailer says {crc:08x}')
			if int(call.consumed[k]) != end - begin:
				raise InflateError(first + k, 'TRAILING_BYTES', f'gzip member {first + k}: {end - begin - int(call.consumed[k])} bytes between the final block and the trailer')
	except BaseException:
		call.free()
		raise
	return call


def _batches(members, max_batch_bytes):
	a = 0
	while a < len(members):
		b, held = a, 0
		while b < len(members):
			size = len(members[b]) + (struct.unpack_from('<I', members[b], len(members[b]) - 4)[0] if len(members[b]) >= 18 else 0)
			if b > a and held + size > max_batch_bytes:
				break
			held += size
			b += 1
		yield a, b
		a = b


def gunzip_many(ctx, members, max_batch_bytes=MAX_BATCH_BYTES):
	"""
	The contents of the gzip members ``members`` (a list of ``bytes``, one member each), inflated on the device of ``ctx`` by its
	calling thread: a list of ``bytes``, in order.  Consecutive members go into one ``tp_inflate`` call until they hold
	``max_batch_bytes`` bytes, compressed and inflated together (a larger member is a call of its own).  Raises :class:`InflateError`,
	naming the member's index and the status, for a stream the decoder does not take to its end, a CRC-32 or an ISIZE that does not
	match, and bytes between the final block and the trailer.
	"""
	members = list(members)
	out = []
	for a, b in _batches(members, max_batch_bytes):
		call = _gunzip_call(ctx, members[a:b], a)
		try:
			out.extend(call.outputs())
		finally:
			call.free()
	return out


def gunzip_to_device(ctx, members):
	"""
	As :func:`gunzip_many` in one call, the contents left on the device: ``(array, offsets)`` -- a uint8 :class:`DeviceArray` (the
	caller frees it) and the uint64 offsets of the ``len(members) + 1`` boundaries in it.  Nothing stays allocated after an error.
	"""
	members = list(members)
	if not members:
		return ctx.empty(4, 'uint8'), np.zeros(1, dtype='uint64')
	call = _gunzip_call(ctx, members, 0)
	try:
		return call.take_output(), call.out_offsets
	finally:
		call.free()
