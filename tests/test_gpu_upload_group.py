# -*- coding: utf-8 -*-
"""
``frameio.upload_group`` on the device: a ``(5, 8, 12)`` float32 memmap of random bit patterns, one frame per chunk -- five chunks, so
both staging buffers are used again -- held bit for bit to the memmap, and a transfer that fails on the third chunk, after which the
allocations on the context, counted at the C entries (tests/alloc_common.py), are back at zero.
"""
import numpy as np
import pytest
from alloc_common import count_allocations
from photometry_amd import frameio
from photometry_amd._lib import TessphotError

pytestmark = pytest.mark.gpu


def test_five_chunks_bit_for_bit_and_a_failed_third_chunk_frees_everything(tmp_path, monkeypatch):
	from photometry_amd.device import Context
	bits = np.random.default_rng(58).integers(0, 2**32, size=(5, 8, 12), dtype='uint64').astype('uint32')
	path = frameio.write_stack(str(tmp_path / 'five.tpstack'), {'images': bits.view('float32')})
	mm = frameio.open_group(path, 'images')
	assert isinstance(mm, np.memmap) and mm.shape == (5, 8, 12) and mm.dtype == np.float32
	with Context(0) as ctx:
		live = count_allocations(ctx, monkeypatch)
		dev = frameio.upload_group(ctx, mm, frames_per_chunk=1)
		assert live == {'device': 1, 'host': 0}, live
		got = dev.to_host()
		assert got.shape == (5, 8, 12) and got.dtype == np.float32 and np.array_equal(got.view('uint32'), bits)
		dev.free()
		assert live == {'device': 0, 'host': 0}, live
		# the third chunk's transfer returns an error: the array, both staging buffers and the events go
		upload, calls = ctx.lib.tp_upload_cube_async, []

		def failing(*args):
			calls.append(args)
			return 1 if len(calls) == 3 else upload(*args)
		monkeypatch.setattr(ctx.lib, 'tp_upload_cube_async', failing)
		with pytest.raises(TessphotError):
			frameio.upload_group(ctx, mm, frames_per_chunk=1)
		assert len(calls) == 3 and live == {'device': 0, 'host': 0}, (len(calls), live)
		monkeypatch.undo()
