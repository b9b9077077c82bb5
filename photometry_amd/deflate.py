# -*- coding: utf-8 -*-
"""
gzip members from the device: many byte strings compressed in one launch (``tp_deflate``, csrc/deflate.hip; the format decisions in
csrc/deflate_rules.h and DESIGN.md section 19).

* :func:`gzip_many` -- a list of byte strings into a list of gzip members: one upload through the context's pooled page-locked
  staging, one ``tp_deflate`` per batch, one download of the chunks' end offsets and CRCs, one download of the packed bytes;
* :func:`gzip_device` -- the same members from byte strings that already lie in a device buffer, given by offsets: no staging, no
  upload (the light-curve files whose table the device wrote, ``lcfile`` with ``table='device'``);
* :func:`deflate_chunks` -- the raw form of one call: the packed deflate bytes of all chunks, their end offsets and their CRCs.

A member is a 10-byte gzip header without FNAME, with ``MTIME = 0`` and ``OS = 255``, the stream's chunks as the device wrote them,
the two bytes ``03 00`` (an empty final fixed block), the stream's CRC-32 (combined from the chunks' CRCs, no pass over the bytes)
and its length: the bytes of a member are a function of its content alone.  They are not zlib's bytes; ``gzip.decompress`` gives
the content back.
"""
import struct
import time as _clock
import numpy as np
from .device import round_up

#: gzip header: magic, CM = 8 (deflate), no flags, MTIME = 0, XFL = 0, OS = 255 (unknown)
GZIP_HEADER = b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff'
#: an empty fixed block with BFINAL: ends the stream behind the last chunk
FINAL_BLOCK = b'\x03\x00'
#: the most input bytes of one ``tp_deflate`` call of :func:`gzip_many` (the call's work buffer takes five times as much)
MAX_BATCH_BYTES = 128 << 20


def chunk_bytes(ctx):
	"""Input bytes of a chunk (``TP_DEFLATE_CHUNK``)."""
	return int(ctx.lib.tp_deflate_chunk_bytes())


class _Lap(object):
	"""Adds the seconds since the last lap to ``parts[name]`` (``parts`` may be None)."""

	def __init__(self, parts):
		self.parts, self.t0 = parts, _clock.perf_counter()

	def __call__(self, name):
		t1 = _clock.perf_counter()
		if self.parts is not None:
			self.parts[name] = self.parts.get(name, 0.0) + t1 - self.t0
		self.t0 = t1


def _call(ctx, blobs, members, parts=None):
	"""One ``tp_deflate`` over ``blobs``.  ``members``: build the gzip members from the page-locked download (one copy per member);
	else return ``(packed bytes, ends, crcs)``.  ``parts``: a dict that receives the seconds of the call's four parts."""
	lap = _Lap(parts)
	lib = ctx.lib
	n = len(blobs)
	offsets = np.zeros(n + 1, dtype='uint64')
	offsets[1:] = np.cumsum([len(b) for b in blobs], dtype='uint64')
	total = int(offsets[-1])
	if total == 0:
		return _device_call(ctx, None, offsets, members, lap)
	words = round_up(total, 4) // 4
	up = ctx.pinned_block(4 * words)
	d_in = None
	try:
		at = 0
		for b in blobs:
			up.array[at:at + len(b)] = np.frombuffer(b, dtype='uint8')
			at += len(b)
		lap('stage')
		d_in = ctx.empty(4 * words, 'uint8')
		ctx._check(lib.tp_upload_cube_async(ctx.handle, d_in.ptr, words, up.ptr, words, 1, words))
		return _device_call(ctx, d_in.ptr, offsets, members, lap, spare=up)
	finally:
		if d_in is not None:
			d_in.free()
		ctx.pinned_release(up)


def _device_call(ctx, d_in_ptr, offsets, members, lap, spare=None):
	"""One ``tp_deflate`` over streams that lie in device memory: stream ``s`` is ``[offsets[s], offsets[s + 1])`` behind ``d_in_ptr``
	(whatever put them there is queued on the context's stream).  ``spare``: a page-locked block that is free once the kernels have
	run and may take the download.  Results as :func:`_call`."""
	lib = ctx.lib
	offsets = np.ascontiguousarray(offsets, dtype='uint64')
	n = len(offsets) - 1
	chunk = chunk_bytes(ctx)
	lens = [int(v) for v in np.diff(offsets.astype('int64'))]
	total = int(offsets[-1]) - int(offsets[0])
	per_stream = [-(-v // chunk) for v in lens]
	n_chunks = sum(per_stream)
	if n_chunks == 0:
		ends, crcs = np.zeros(0, dtype='uint64'), np.zeros(0, dtype='uint32')
		return [_member([], 0, 0)] * n if members else (b'', ends, crcs)
	capacity = total + 5 * n_chunks                                    # the sum of tp_deflate_bound over the streams
	work_bytes = int(lib.tp_deflate_work_bytes(offsets.ctypes.data, n))
	meta = ctx.pinned_block(12 * n_chunks)
	down = None
	d_out = d_meta = d_work = None
	try:
		d_out = ctx.empty(capacity, 'uint8')
		d_meta = ctx.empty(12 * n_chunks, 'uint8')                      # n_chunks ends (uint64), then n_chunks CRCs (uint32)
		d_work = ctx.empty(work_bytes, 'uint8')
		ctx._check(lib.tp_deflate(ctx.handle, d_in_ptr, offsets.ctypes.data, n, d_out.ptr, capacity, d_meta.ptr, d_meta.ptr + 8 * n_chunks, d_work.ptr, work_bytes))
		ctx.download_async(meta, d_meta, nbytes=12 * n_chunks)
		ctx.sync()
		ends = np.array(meta.array[:8 * n_chunks].view('uint64'))
		crcs = np.array(meta.array[8 * n_chunks:12 * n_chunks].view('uint32'))
		packed_bytes = int(ends[-1])
		assert packed_bytes <= capacity
		lap('upload_and_kernels')
		down = spare if spare is not None and spare.nbytes >= packed_bytes else ctx.pinned_block(packed_bytes)   # (the upload is over: its block takes the download)
		ctx.download_async(down, d_out, nbytes=packed_bytes)
		ctx.sync()
		packed = memoryview(down.array)[:packed_bytes]
		lap('download')
		if not members:
			return bytes(packed), ends, crcs
		out = []
		c, begin = 0, 0
		for nbytes, k in zip(lens, per_stream):
			end = int(ends[c + k - 1]) if k else begin
			crc = 0
			for j in range(k):
				crc = lib.tp_crc32_combine(crc, int(crcs[c + j]), min(chunk, nbytes - j * chunk))
			out.append(_member([packed[begin:end]], crc, nbytes))
			c, begin = c + k, end
		lap('members')
		return out
	finally:
		for d in (d_out, d_meta, d_work):
			if d is not None:
				d.free()
		ctx.pinned_release(meta)
		if down is not None and down is not spare:
			ctx.pinned_release(down)


def _member(pieces, crc, nbytes):
	return b''.join([GZIP_HEADER] + pieces + [FINAL_BLOCK, struct.pack('<II', crc & 0xFFFFFFFF, nbytes & 0xFFFFFFFF)])


def deflate_chunks(ctx, blobs):
	"""
	One ``tp_deflate`` call over the byte strings ``blobs`` as its streams: ``(packed, ends, crcs)`` -- the deflate bytes of all chunks
	back to back, the end offset of every chunk in them (uint64) and the CRC-32 of every chunk's input (uint32), the chunks in call
	order (a stream of ``n`` bytes has ``ceil(n / chunk_bytes)`` of them).  A stream's chunks followed by ``03 00`` are a raw deflate stream.
	"""
	return _call(ctx, [bytes(b) for b in blobs], members=False)


def gzip_many(ctx, blobs, max_batch_bytes=MAX_BATCH_BYTES, parts=None):
	"""
	The byte strings ``blobs`` as gzip members (a list of ``bytes``, in order), compressed on the device of ``ctx`` by its calling
	thread.  Consecutive blobs go into one ``tp_deflate`` call until they hold ``max_batch_bytes`` bytes of input (a larger blob is a
	call of its own); the device memory of a call is about six times its input.  An empty blob gives a valid, empty member.
	``parts``: a dict that receives the seconds spent in ``stage`` (the blobs into page-locked memory), ``upload_and_kernels`` (up to
	the download of offsets and CRCs), ``download`` (the packed bytes) and ``members`` (CRCs combined, members joined).
	"""
	blobs = list(blobs)
	out = []
	a = 0
	while a < len(blobs):
		b, held = a, 0
		while b < len(blobs) and (b == a or held + len(blobs[b]) <= max_batch_bytes):
			held += len(blobs[b])
			b += 1
		out.extend(_call(ctx, blobs[a:b], members=True, parts=parts))
		a = b
	return out


def gzip_device(ctx, d_in, offsets, max_batch_bytes=MAX_BATCH_BYTES, parts=None):
	"""
	:func:`gzip_many` for byte strings that already lie in device memory: string ``s`` is ``[offsets[s], offsets[s + 1])`` of the
	uint8 device array ``d_in`` (``offsets``: ``n + 1`` values that do not fall; what filled ``d_in`` is queued on the context's
	stream).  The same members, batches and ``parts`` as :func:`gzip_many` without ``stage``: nothing is staged or uploaded.
	"""
	offsets = np.ascontiguousarray(offsets, dtype='uint64')
	n = len(offsets) - 1
	if n < 0 or (n and int(offsets[-1]) > d_in.nbytes) or np.any(np.diff(offsets.astype('int64')) < 0):
		raise ValueError("offsets must be n + 1 values inside the device array that do not fall")
	lap = _Lap(parts)
	out = []
	a = 0
	while a < n:
		b = a + 1
		while b < n and int(offsets[b + 1]) - int(offsets[a]) <= max_batch_bytes:
			b += 1
		out.extend(_device_call(ctx, d_in.ptr, offsets[a:b + 1], True, lap))
		a = b
	return out
