# -*- coding: utf-8 -*-
"""
``tp_star_positions_targets`` (csrc/starpos.hip) against the numpy restatement of tests/tpf_linpsf_common.py, bit for bit: five targets
with 1, 3, 1, 4 and 2 stars, the stars of a target not adjacent; ``T = 300`` (two blocks along the cadences, the second partial) and
``T = 1``; ``pos_pitch = 320 > T`` with the tail of every row pre-filled and found untouched; shifts of 1e-3 .. 0.3 px beside bases
near 5.5, so the float32 sum rounds; one target with NaN shifts at three cadences; one target with a lookup that repeats a row --
passed as a whole array with identity rows, and as the batch passes it: NULL for every star, then that target's stars again.
"""
import numpy as np
import pytest
import tpf_linpsf_common as lc
from photometry_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _prefilled(ctx, n, pitch):
	return ctx.array(np.full((n, pitch), lc.SENTINEL_BITS, dtype='uint64').view('float64'))


@pytest.mark.parametrize('T,pitch', [(300, 320), (1, 320), (1, 1)])
def test_kernel_equals_the_restatement(ctx, T, pitch):
	base, star_target, shift, lookup = lc.kernel_case(T=T, pos_pitch=pitch)
	assert sorted(np.bincount(star_target).tolist()) == [1, 1, 2, 3, 4] and not np.any(star_target[1:] == star_target[:-1])
	n = len(base)
	d_base, d_tgt, d_shift = ctx.array(base), ctx.array(star_target), ctx.array(shift)
	# NULL: identity for every target
	d_pos = _prefilled(ctx, n, pitch)
	engine.star_positions_targets(ctx, d_base, d_tgt, d_shift, T, out=d_pos)
	want = lc.positions_numpy(base, star_target, shift, T, pos_pitch=pitch)
	got = d_pos.to_host()
	np.testing.assert_array_equal(lc.bits(got), lc.bits(want))
	assert np.all(lc.bits(got[:, T:]) == lc.SENTINEL_BITS)
	assert np.isnan(got[star_target == 1, :T]).sum() == 3 * len({0, T // 2, T - 1})
	assert np.any(got[:, :T] != base[:, None].astype('float64') + shift[star_target])       # the float32 sum rounds
	# a whole lookup array: identity rows but for target 3
	whole = np.stack([np.arange(T, dtype='int32') if v is None else v for v in lookup]).astype('int32')
	d_look = ctx.array(whole)
	d_pos2 = _prefilled(ctx, n, pitch)
	engine.star_positions_targets(ctx, d_base, d_tgt, d_shift, T, lookup=d_look, out=d_pos2)
	want2 = lc.positions_numpy(base, star_target, shift, T, lookup=lookup, pos_pitch=pitch)
	np.testing.assert_array_equal(lc.bits(d_pos2.to_host()), lc.bits(want2))
	if T > 3:
		assert np.any(lc.bits(want2) != lc.bits(want))
	# as the batch does it: NULL for all (d_pos), then the stars of the target with a lookup again, one series and one lookup row
	d_one, d_zero = ctx.array(whole[3:4]), ctx.array(np.zeros(1, dtype='int32'))
	for s in np.flatnonzero(star_target == 3):
		engine.star_positions_targets(ctx, d_base.slice0(s, 1), d_zero, d_shift.slice0(3, 1), T, lookup=d_one, out=d_pos.slice0(s, 1))
	np.testing.assert_array_equal(lc.bits(d_pos.to_host()), lc.bits(want2))


def test_more_stars_than_one_launch_row(ctx):
	"""Stars beyond gridDim.y = 65535 are walked by the blocks of the first ones."""
	rng = np.random.default_rng(2)
	n, T = 65535 + 70, 3
	base = rng.normal(size=n).astype('float32') + 5
	star_target = rng.integers(0, 4, size=n).astype('int32')
	shift = rng.uniform(-0.3, 0.3, size=(4, T))
	got = engine.star_positions_targets(ctx, ctx.array(base), ctx.array(star_target), ctx.array(shift), T).to_host()
	want = (base[:, None] + shift[star_target].astype('float32')).astype('float64')
	np.testing.assert_array_equal(lc.bits(got), lc.bits(want))


def test_bad_sizes_and_null_pointers_return_the_error(ctx):
	from photometry_amd._lib import TessphotError
	base, star_target, shift, _ = lc.kernel_case(T=8)
	d_base, d_tgt, d_shift, d_pos = ctx.array(base), ctx.array(star_target), ctx.array(shift), _prefilled(ctx, len(base), 8)
	d_look = ctx.array(np.zeros((5, 8), dtype='int32'))
	lib, h = ctx.lib, ctx.handle

	def call(n_stars=len(base), n_cad=8, base_p=d_base.ptr, tgt_p=d_tgt.ptr, shift_p=d_shift.ptr, shift_pitch=8, look_p=None, look_pitch=0, n_targets=5, pos_p=d_pos.ptr, pos_pitch=8):
		return lib.tp_star_positions_targets(h, n_stars, n_cad, base_p, tgt_p, shift_p, shift_pitch, look_p, look_pitch, n_targets, pos_p, pos_pitch)
	assert call() == 0
	ctx.sync()
	before = d_pos.to_host()
	for kw in (dict(n_stars=-1), dict(n_cad=-1), dict(pos_pitch=7), dict(shift_pitch=7), dict(n_targets=0), dict(look_p=d_look.ptr, look_pitch=7),
			dict(look_p=d_look.ptr, look_pitch=8, shift_pitch=0), dict(base_p=None), dict(tgt_p=None), dict(shift_p=None), dict(pos_p=None)):
		assert call(**kw) != 0, kw
		with pytest.raises(TessphotError, match='tp_star_positions_targets'):
			ctx._check(call(**kw))
	assert call(n_stars=0, base_p=None) == 0 and call(n_cad=0, pos_p=None) == 0       # nothing to do: no pointer is looked at
	ctx.sync()
	np.testing.assert_array_equal(lc.bits(d_pos.to_host()), lc.bits(before))            # no refused call launched anything
