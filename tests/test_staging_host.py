# -*- coding: utf-8 -*-
"""
``photometry_amd.staging`` without a GPU: :class:`StagedUpload` driven with a fake ``ctx`` and a fake transfer context that append every
call to one log.  Held on the log: the order of the calls per item, that no staging buffer is filled before the event recorded behind
its previous upload has been waited on, and that leaving the ``with`` block syncs the transfer context before anything is freed,
destroys both events and frees everything exactly once, whatever was raised and wherever.
"""
import gzip
import numpy as np
import pytest
from photometry_amd import ffi, staging

STAGE, SLOT = 64, 64
STAGE_PTR, SLOT_PTR, SUMS_PTR = (0x1000, 0x2000), 0x8000, 0x9000
EVENTS = (101, 102)


class FakeArray(object):
	def __init__(self, log, name, ptr, shape, dtype):
		self.log, self.name, self.ptr, self.shape = log, name, ptr, tuple(shape)
		self.array = np.zeros(shape, dtype=dtype)

	def free(self):
		self.log.append(('free', self.name))

	def to_host(self):
		return self.array


class FakeCtx(object):
	device = 3

	def __init__(self, log):
		self.log, self.n_pinned = log, 0

	def pinned(self, shape, dtype):
		k = self.n_pinned
		self.n_pinned += 1
		self.log.append(('pinned', k))
		return FakeArray(self.log, 'stage%d' % k, STAGE_PTR[k], shape, dtype)

	def empty(self, shape, dtype):
		self.log.append(('empty', tuple(shape)))
		return FakeArray(self.log, 'slots', SLOT_PTR, shape, dtype)

	def zeros(self, shape, dtype):
		self.log.append(('zeros', tuple(shape)))
		return FakeArray(self.log, 'sums', SUMS_PTR, shape, dtype)

	def sync(self):
		self.log.append(('sync', 'ctx'))


class FakeLib(object):
	def __init__(self, log):
		self.log = log

	def tp_upload_cube_async(self, handle, dst, pitch, src, src_pitch, rows, n):
		assert pitch == src_pitch == n and rows == 1
		s = 0 if src < STAGE_PTR[1] else 1
		self.log.append(('upload', s, src - STAGE_PTR[s], dst - SLOT_PTR, 4 * n))
		return 0

	def tp_fits_datasum(self, handle, src, nbytes, dst):
		self.log.append(('datasum', src - SLOT_PTR, nbytes, (dst - SUMS_PTR) // 8))
		return 0

	def tp_event_destroy(self, handle, event):
		self.log.append(('tp_event_destroy', event))
		return 0


class FakeUp(object):
	"""``fail_syncs``: how many of the first ``sync`` calls raise."""

	def __init__(self, log, fail_syncs=0):
		self.log, self.lib, self.handle, self.n_events, self.fail_syncs = log, FakeLib(log), 77, 0, fail_syncs

	def _check(self, rc):
		assert rc == 0

	def event(self):
		e = EVENTS[self.n_events]
		self.n_events += 1
		self.log.append(('event', e))
		return e

	def event_sync(self, event):
		self.log.append(('event_sync', event))

	def record(self, event):
		self.log.append(('record', event))

	def sync(self):
		self.log.append(('sync', 'up'))
		if self.fail_syncs > 0:
			self.fail_syncs -= 1
			raise RuntimeError('sync failed')

	def close(self):
		self.log.append(('close', 'up'))
		self.handle = None


class Boom(Exception):
	pass


def drive(st, log, n_items, boom=None):
	"""The loop body of a loader with two uploads per item; ``boom``: ``('fill', i)`` or ``('uploaded', i)`` raises there."""
	def fill(i, buf):
		log.append(('fill', 0 if buf is stages[0] else 1))
		if boom == ('fill', i):
			raise Boom()
		buf[:] = i + 1
	stages = [p.array for p in st.stage]
	for i in range(n_items):
		st.take()
		st.fill(lambda buf: fill(i, buf)) # noqa: B023
		assert np.all(st.buf.array == i + 1)
		st.upload(st.slot, 32)
		st.upload(st.slot + 32, 32, offset=32)
		if boom == ('uploaded', i):
			raise Boom()
		st.record()
		st.datasum(st.slot, 64, i)
		log.append(('kernel', i))
	return st.finish()


SETUP = [('empty', (2, SLOT)), ('zeros', None), ('sync', 'ctx'), ('pinned', 0), ('pinned', 1), ('event', EVENTS[0]), ('event', EVENTS[1])]
TEARDOWN = [('sync', 'up'), ('tp_event_destroy', EVENTS[0]), ('tp_event_destroy', EVENTS[1]), ('free', 'stage0'), ('free', 'stage1'), ('free', 'slots'), ('free', 'sums')]


def expected(n_items):
	"""Today's order: slots, sums, ``ctx.sync``, buffers, events; per item wait (from the third on), fill, uploads, record, datasum and
	the loader's kernel; the final sync; then the four steps of ``__exit__``."""
	log = [c if c[0] != 'zeros' else ('zeros', (n_items,)) for c in SETUP]
	for i in range(n_items):
		s = i % 2
		if i >= 2:
			log.append(('event_sync', EVENTS[s]))
		log += [('fill', s), ('upload', s, 0, s * SLOT, 32), ('upload', s, 32, s * SLOT + 32, 32), ('record', EVENTS[s]), ('datasum', s * SLOT, 64, i), ('kernel', i)]
	return log + [('sync', 'up')] + TEARDOWN


def check_buffer_reuse(log):
	"""Buffer ``s`` is never filled before the event recorded after its previous upload has been waited on."""
	state = {0: 'free', 1: 'free'}      # free -> filled -> (uploads) -> recorded -> free again through event_sync
	for call in log:
		if call[0] == 'fill':
			assert state[call[1]] == 'free', (call, state)
			state[call[1]] = 'filled'
		elif call[0] == 'upload':
			assert state[call[1]] == 'filled', (call, state)
		elif call[0] == 'record':
			assert state[EVENTS.index(call[1])] == 'filled', (call, state)
			state[EVENTS.index(call[1])] = 'recorded'
		elif call[0] == 'event_sync':
			assert state[EVENTS.index(call[1])] == 'recorded', (call, state)
			state[EVENTS.index(call[1])] = 'free'


def check_teardown(log, closed):
	"""A sync of ``up`` precedes every free and every destroy; events, buffers, slots and sums go exactly once; ``close`` comes last, if at all."""
	first = min(k for k, c in enumerate(log) if c[0] in ('free', 'tp_event_destroy'))
	assert ('sync', 'up') in log[:first] and log[first - 1] == ('sync', 'up')
	assert sorted(c for c in log if c[0] in ('free', 'tp_event_destroy')) == sorted(TEARDOWN[1:])
	assert log.count(('close', 'up')) == (1 if closed else 0)
	assert log[-len(TEARDOWN) - closed:] == TEARDOWN + [('close', 'up')] * closed


@pytest.mark.parametrize('n_items', [1, 2, 3, 5])
def test_the_log_of_a_run_is_todays_order(n_items):
	log = []
	up = FakeUp(log)
	with staging.StagedUpload(FakeCtx(log), STAGE, SLOT, n_items, up=up) as st:
		assert st.up is up and st.stats == {'read_s': 0.0, 'wait_s': 0.0}
		mine = st.stats = {'read_s': 0.0, 'wait_s': 0.0, 'bytes': 5}
		sums = drive(st, log, n_items)
		assert sums.shape == (n_items,) and sums.dtype == np.uint64
		assert st.stats is mine and mine['read_s'] > 0 and mine['wait_s'] > 0 and mine['bytes'] == 5
	assert log == expected(n_items)
	check_buffer_reuse(log)
	check_teardown(log, closed=False)
	assert [c for c in log if c[0] == 'event_sync'] == [('event_sync', EVENTS[i % 2]) for i in range(2, n_items)]


def test_without_slots_and_sums_nothing_is_allocated_for_them():
	log = []
	with staging.StagedUpload(FakeCtx(log), STAGE, up=FakeUp(log)) as st:
		st.take()
		assert st.slot is None
		st.fill(lambda buf: None)
		st.upload(SLOT_PTR + 8, 16)
		st.record()
		assert st.finish() is None
	assert log == [('sync', 'ctx'), ('pinned', 0), ('pinned', 1), ('event', EVENTS[0]), ('event', EVENTS[1]), ('upload', 0, 0, 8, 16), ('record', EVENTS[0]),
		('sync', 'up'), ('sync', 'up'), ('tp_event_destroy', EVENTS[0]), ('tp_event_destroy', EVENTS[1]), ('free', 'stage0'), ('free', 'stage1')]


@pytest.mark.parametrize('boom,fail_syncs', [(('fill', 0), 0), (('uploaded', 1), 0), (None, 1), (None, 2)])
def test_an_exception_anywhere_leaves_nothing_behind(boom, fail_syncs):
	"""In the fill of item 0, after the uploads of item 1, in ``finish`` -- and in ``finish`` with the sync of ``__exit__`` failing too."""
	log = []
	with pytest.raises(Boom if boom else RuntimeError):
		with staging.StagedUpload(FakeCtx(log), STAGE, SLOT, 3, up=FakeUp(log, fail_syncs)) as st:
			drive(st, log, 3, boom=boom)
	if boom == ('fill', 0):
		assert not any(c[0] in ('upload', 'record', 'datasum', 'kernel') for c in log)
	elif boom == ('uploaded', 1):
		assert [c for c in log if c[0] in ('upload', 'record')][-3:] == [('record', EVENTS[0]), ('upload', 1, 0, SLOT, 32), ('upload', 1, 32, SLOT + 32, 32)]
	else:
		assert log.count(('sync', 'up')) == 2 and log.count(('kernel', 2)) == 1
	check_buffer_reuse(log)
	check_teardown(log, closed=False)


@pytest.mark.parametrize('boom', [None, ('uploaded', 1)])
def test_an_own_transfer_context_is_made_after_the_sync_and_closed_last(monkeypatch, boom):
	log, made = [], []

	def context(device, high_priority=None):
		made.append((device, high_priority))
		log.append(('context', device))
		return FakeUp(log)
	monkeypatch.setattr(staging, 'Context', context)
	try:
		with staging.StagedUpload(FakeCtx(log), STAGE, SLOT, 2) as st:
			drive(st, log, 2, boom=boom)
	except Boom:
		assert boom is not None
	assert made == [(FakeCtx.device, False)]                              # the low-priority stream of ctx's device
	assert log[:4] == [('empty', (2, SLOT)), ('zeros', (2,)), ('sync', 'ctx'), ('context', FakeCtx.device)]
	if boom is None:
		assert [c for c in log if c[0] != 'context'] == expected(2) + [('close', 'up')]
	check_teardown(log, closed=True)


def test_a_failure_while_setting_up_frees_what_there_is(monkeypatch):
	log = []

	class Ctx(FakeCtx):
		def pinned(self, shape, dtype):
			if self.n_pinned == 1:
				raise MemoryError('no page-locked memory')
			return FakeCtx.pinned(self, shape, dtype)
	monkeypatch.setattr(staging, 'Context', lambda device, high_priority=None: FakeUp(log))
	with pytest.raises(MemoryError):
		staging.StagedUpload(Ctx(log), STAGE, SLOT, 4)
	assert log == [('empty', (2, SLOT)), ('zeros', (4,)), ('sync', 'ctx'), ('pinned', 0), ('sync', 'up'), ('free', 'stage0'), ('free', 'slots'), ('free', 'sums'), ('close', 'up')]


# ---- the reader and the checksum refusal ---------------------------------------------------------------------------------------------
def test_read_fills_the_buffer_from_a_plain_and_a_gz_file(tmp_path):
	blob = bytes(np.random.default_rng(1).integers(0, 256, 300, dtype='uint8'))
	plain, gz = str(tmp_path / 'a.bin'), str(tmp_path / 'a.bin.gz')
	with open(plain, 'wb') as fh:
		fh.write(blob)
	with gzip.open(gz, 'wb') as fh:
		fh.write(blob)
	log = []
	with staging.StagedUpload(FakeCtx(log), STAGE, up=FakeUp(log)) as st:
		for path in (plain, gz):
			st.take()
			st.read(path, 100, 40)
			assert bytes(st.buf.array[:40]) == blob[100:140] and not st.buf.array[40:].any()
		assert st.stats['read_s'] > 0
		with pytest.raises(ValueError, match=r'a\.bin: the file ends inside a data unit \(300 of 310 bytes\)'):
			st.read(plain, 250, 60)
	buf = np.zeros(16, dtype='uint8')
	staging.read_into(gz, buf, 290, 10)
	assert bytes(buf[:10]) == blob[290:] and not buf[10:].any()


def test_check_datasum_raises_the_loaders_text():
	staging.check_datasum('x.fits', 1, np.uint64(7), 7)
	staging.check_datasum('x.fits', 1, np.uint64(7), None)                # no DATASUM card: nothing to hold the sum to
	with pytest.raises(ffi.ChecksumError) as e:
		staging.check_datasum('dir/x.fits', 2, np.uint64(8), 7)
	assert str(e.value) == "dir/x.fits: HDU 2: the data unit sums to 8, its DATASUM card says 7" and isinstance(e.value, ValueError)
