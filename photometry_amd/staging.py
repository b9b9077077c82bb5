# -*- coding: utf-8 -*-
"""
Staged uploads: the one overlap scheme of the loaders (``frameio.upload_group``, ``ffi.load_ffis``, ``tpf.load_tpfs``,
``tpf.load_tpf_groups``).

Items (files, chunks of frames) pass through two page-locked staging buffers on a second, low-priority context: while item ``i``
travels over the link and is unpacked, the host fills the other buffer with item ``i + 1``.  An event per buffer, recorded behind the
last upload out of it, is waited on before the buffer is filled again.  Per item a loader calls :meth:`StagedUpload.take`,
:meth:`~StagedUpload.read` or :meth:`~StagedUpload.fill`, :meth:`~StagedUpload.upload` (as often as it has pieces),
:meth:`~StagedUpload.record`, then queues its own kernels on ``up``; :meth:`~StagedUpload.finish` waits for everything.

Leaving the ``with`` block syncs the transfer context before anything is freed, whatever happened.  A loader therefore frees its own
outputs in an ``except`` *around* the ``with``: nothing is still queued that could write into a block the allocation cache hands out again.
"""

import time as _time
from . import fitsio
from .device import Context


def read_into(path, buf, start, nbytes):
	"""``nbytes`` of the (decompressed) file from byte ``start`` into the uint8 array ``buf``, without an intermediate copy."""
	view = memoryview(buf)[:nbytes]
	with fitsio.opener(path)(path, 'rb') as fh:
		fh.seek(start)
		got = 0
		while got < nbytes:
			n = fh.readinto(view[got:])
			if not n:
				raise ValueError(f"{path}: the file ends inside a data unit ({start + got} of {start + nbytes} bytes)")
			got += n


def check_datasum(path, hdu, got, want):
	"""Raise ``ffi.ChecksumError`` unless the word sum ``got`` of a data unit is its ``DATASUM`` card ``want`` (None: no card)."""
	from .ffi import ChecksumError
	if want is not None and int(got) != want:
		raise ChecksumError(f"{path}: HDU {hdu}: the data unit sums to {int(got)}, its DATASUM card says {want}")


class StagedUpload(object):
	"""
	Two page-locked buffers of ``stage_bytes`` (allocated on ``ctx``), an event each, two device slots of ``slot_bytes`` (0: none),
	``n_sums`` zeroed uint64 word sums (0: none) and the transfer context ``up`` (a borrowed one is not closed).  ``ctx`` is synced
	before the transfer context is made, so what the caller allocated on it exists before the other stream writes it.

	``buf``: the staging buffer of the current item (a :class:`~photometry_amd.device.PinnedArray`), ``slot``: the device address of
	its slot; ``stats``: seconds in ``read_s`` / ``wait_s`` (a loader may put a dict of its own there per item).
	"""

	def __init__(self, ctx, stage_bytes, slot_bytes=0, n_sums=0, up=None):
		self.up, self._own = up, up is None
		self.stage, self.done, self.slots, self.sums = [], [], None, None
		self.stats = {'read_s': 0.0, 'wait_s': 0.0}
		self._n = 0
		try:
			if slot_bytes:
				self.slots = ctx.empty((2, slot_bytes), 'uint8')
			if n_sums:
				self.sums = ctx.zeros((n_sums,), 'uint64')
			ctx.sync()
			if self._own:
				self.up = Context(ctx.device, high_priority=False)
			for _ in range(2):
				self.stage.append(ctx.pinned((stage_bytes,), 'uint8'))   # (one at a time: the first is not lost when the second fails)
			for _ in range(2):
				self.done.append(self.up.event())
		except BaseException:
			self.__exit__()
			raise

	def __enter__(self):
		return self

	def __exit__(self, *exc):
		up = self.up
		if up is not None and getattr(up, 'handle', None) is not None:
			try:
				up.sync()
			except Exception: # noqa: B902
				pass
			for e in self.done:
				up.lib.tp_event_destroy(up.handle, e)
		for a in self.stage + [self.slots, self.sums]:
			if a is not None:
				a.free()
		if self._own and up is not None:
			up.close()
		self.stage, self.done, self.slots, self.sums, self.up = [], [], None, None, None

	def take(self):
		"""Make the next staging buffer the current one; from the third item on, wait until the uploads that last read it are over."""
		s = self._n % 2
		if self._n >= 2:
			t0 = _time.perf_counter()
			self.up.event_sync(self.done[s])
			self.stats['wait_s'] += _time.perf_counter() - t0
		self._n += 1
		self._s, self.buf = s, self.stage[s]
		self.slot = None if self.slots is None else self.slots.ptr + s * self.slots.shape[1]

	def fill(self, copy):
		"""``copy(array)`` writes the item into the current buffer (uint8): page cache / disk -> pinned memory, while item ``i - 1`` is in flight."""
		t0 = _time.perf_counter()
		copy(self.buf.array)
		self.stats['read_s'] += _time.perf_counter() - t0

	def read(self, path, start, nbytes):
		"""Fill the current buffer with ``nbytes`` of the file ``path`` from byte ``start`` (:func:`read_into`)."""
		self.fill(lambda buf: read_into(path, buf, start, nbytes))

	def upload(self, dst, nbytes, offset=0):
		"""Queue the copy of ``nbytes`` (a multiple of 4) from byte ``offset`` of the current buffer to the device address ``dst``."""
		up = self.up
		up._check(up.lib.tp_upload_cube_async(up.handle, dst, nbytes // 4, self.buf.ptr + offset, nbytes // 4, 1, nbytes // 4))

	def record(self):
		"""Record the current buffer's event: behind the last upload out of it."""
		self.up.record(self.done[self._s])

	def datasum(self, src, nbytes, k):
		"""Queue ``tp_fits_datasum`` of the device range ``[src, src + nbytes)`` into sum ``k``."""
		self.up._check(self.up.lib.tp_fits_datasum(self.up.handle, src, nbytes, self.sums.ptr + 8 * k))

	def finish(self):
		"""Wait for everything queued on the transfer context; returns the word sums on the host (None without any)."""
		t0 = _time.perf_counter()
		self.up.sync()
		self.stats['wait_s'] += _time.perf_counter() - t0
		return None if self.sums is None else self.sums.to_host()
