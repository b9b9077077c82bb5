# -*- coding: utf-8 -*-
"""
CPU checks of the image-motion host layer that never reach the device: an image whose shape differs from the reference gives the
reference's NaN kernel (and no launch); a template of another geometry than the frames is refused before tp_motion_ecc; a
``.tpstack`` header written without a reference frame builds its MovementKernel; every motion kernel has its own profile entry.
"""
import logging
import numpy as np
import pytest
from photometry_amd import motion


class _NoDevice(object):
	"""A context stand-in that fails the test on any use."""
	def __getattr__(self, name):
		raise AssertionError(f"the device was used: ctx.{name}")


class _Shape(object):
	def __init__(self, shape):
		self.shape = shape
		self.ptr = 0
		self.dtype = np.dtype('float32')


@pytest.mark.parametrize('mode', ['translation', 'euclidian', 'affine'])
@pytest.mark.parametrize('shape', [(12, 10), (10, 12), (8, 10), (2, 10, 10), (100,)])
def test_calc_kernel_other_shape_is_nan_without_device(mode, shape, caplog):
	mk = motion.MovementKernel(mode, image_ref=np.ones((10, 10)), ctx=_NoDevice())
	with caplog.at_level(logging.ERROR, logger='photometry_amd.motion'):
		k = mk.calc_kernel(np.ones(shape, dtype='float32'))
	assert len(k) == mk.n_params and np.all(np.isnan(k))
	assert any('Could not find transform' in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize('tshape', [(1, 12, 10), (12, 10), (1, 10, 12), (2, 10, 10), (10,)])
def test_ecc_prepared_refuses_template_of_other_geometry(tshape):
	with pytest.raises(ValueError, match='does not match the frames'):
		motion.ecc_prepared(_NoDevice(), _Shape(tshape), _Shape((3, 10, 10)), 'translation')


def test_header_without_ref_frame(tmp_path):
	from photometry_amd import frameio
	T = 5
	kernels = np.random.default_rng(4).normal(0, 0.2, (T, 2))
	time = 1500.0 + np.arange(T) / 48.0
	path = frameio.write_stack(str(tmp_path / 'n.tpstack'), {'images': np.zeros((T, 4, 4), dtype='float32')}, time=time, movement_kernel=kernels)
	hdr = frameio.read_header(path)
	assert hdr['attrs']['movement_kernel']['ref_frame'] is None
	mk = motion.movement_from_header(hdr)
	assert mk.ref_frame is None and mk.warpmode == 'translation'
	np.testing.assert_allclose(mk.jitter(time, 3.0, 4.0), kernels, rtol=0, atol=1e-12)   # interp1d at the nodes


def test_motion_kernels_have_profile_entries():
	import __graft_entry__ as g
	g.build()
	from photometry_amd import _lib
	lib = _lib.load()
	names = [lib.tp_kernel_name(k).decode() for k in range(lib.tp_kernel_count())]
	for n in ('tp_motion_prepare_kernel', 'tp_motion_minmax_kernel', 'tp_motion_blur_kernel', 'tp_motion_init_kernel',
		'tp_motion_iter_kernel', 'tp_motion_finish_kernel'):
		assert names.count(n) == 1, n
