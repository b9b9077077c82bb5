# -*- coding: utf-8 -*-
"""
The cases of the per-stamp flag series (``tp_stamp_flag_series``; csrc/stampflags.hip, csrc/stampflags_rules.h), shared by the host
check of the rules (tests/test_stampflags_host.py) and the GPU test of the C ABI (tests/test_gpu_stamp_flags.py), with the numpy
line both are held to: ``np.any(flags[:, r1:r2, c1:c2] & bit, axis=(1, 2))`` -- save_lightcurve's reduction (BasePhotometry.py:1445-1449).
"""
import numpy as np

BIT = 4             # PixelQualityFlags.BackgroundShenanigans
OUT_VALUE = 256     # CorrectorQualityFlags.BackgroundShenanigans
SENTINEL = -123456789
ROW0, COL0 = 17, 44
REGIONS = [(5, 7), (40, 130)]
NO_STAMP = (-1, -1, -1, -1)


def region_stamps(R, C):
	"""The stamps of one call, relative to the region: (r1, r2, c1, c2)."""
	st = [(0, 1, 0, 1), (0, 1, C - 1, C), (R - 1, R, 0, 1), (R - 1, R, C - 1, C),      # 1 x 1 in each corner
		(0, R, 0, C),                                                                  # the whole region
		(R // 2, R // 2 + 1, 0, C),                                                    # a full row (1 x 130: wider than two wavefronts)
		(0, R, C // 2, C // 2 + 1)]                                                    # a full column
	for w in range(1, 10):                                                             # widths 1..9 at column offsets 0..3 mod 4
		for off in range(4):
			if off + w <= C:
				r = (w + off) % max(R - 2, 1)
				st.append((r, min(r + 3, R), off, off + w))
	st.append(NO_STAMP)
	st += [(1, 4, 2, 6), (1, 4, 2, 6)]                                                 # the same stamp twice
	return np.asarray(st, dtype='int64')


def to_ccd(stamps):
	st = np.array(stamps, dtype='int64', copy=True)
	real = ~np.all(st == -1, axis=1)
	st[real] += np.array([ROW0, ROW0, COL0, COL0])
	return st


def make_flags(kind, T, R, C, seed=0):
	rng = np.random.default_rng(seed)
	if kind == 'clear':
		return np.zeros((T, R, C), dtype='uint8')
	if kind == 'other_bits':
		return np.full((T, R, C), 0xFB, dtype='uint8')
	if kind == 'sparse':
		f = rng.integers(0, 4, (T, R, C)).astype('uint8')              # (bits 1 and 2 everywhere, bit 4 at density 1e-3)
		f[rng.random((T, R, C)) < 1e-3] |= BIT
		return f
	if kind == 'everywhere':
		return np.full((T, R, C), BIT, dtype='uint8')
	raise ValueError(kind)


def with_stride(flags, pad):
	"""The stack as the bytes a call may read: frames ``R * C + pad`` bytes apart, the bytes between two frames 0xFF."""
	T, R, C = flags.shape
	stride = R * C + pad
	raw = np.full((T - 1) * stride + R * C, 0xFF, dtype='uint8')
	for t in range(T):
		raw[t * stride:t * stride + R * C] = flags[t].ravel()
	return raw, stride


def expected(flags, stamps, bit=BIT, out_value=OUT_VALUE):
	T = flags.shape[0]
	out = np.zeros((len(stamps), T), dtype='int32')
	for i, (r1, r2, c1, c2) in enumerate(stamps):
		if (r1, r2, c1, c2) == NO_STAMP:
			continue
		out[i, np.any(flags[:, r1:r2, c1:c2] & bit, axis=(1, 2))] = out_value
	return out


def neighbours_case():
	"""A stamp with a flagged pixel just outside each of its four sides and at each outer corner, one per frame (frame 8: all eight;
	frame 9: one inside), every other bit set everywhere."""
	R, C = 40, 130
	r1, r2, c1, c2 = 10, 15, 61, 70
	around = [(r1 - 1, c1 + 2), (r2, c1 + 2), (r1 + 2, c1 - 1), (r1 + 2, c2), (r1 - 1, c1 - 1), (r1 - 1, c2), (r2, c1 - 1), (r2, c2)]
	flags = np.full((10, R, C), 0xFB, dtype='uint8')
	for t, (r, c) in enumerate(around):
		flags[t, r, c] |= BIT
		flags[8, r, c] |= BIT
	flags[9, r2 - 1, c2 - 1] |= BIT
	stamps = np.asarray([(r1, r2, c1, c2), (r1 - 1, r2 + 1, c1 - 1, c2 + 1)], dtype='int64')
	return flags, stamps


def single_frames_case():
	"""65 frames: frame 16 flagged inside the stamps with clean neighbours, frame 31 with the frame's first pixel alone, frame 64 with
	its last pixel alone."""
	R, C = 40, 130
	flags = np.zeros((65, R, C), dtype='uint8')
	flags[16, 20, 64] = BIT
	flags[31, 0, 0] = BIT
	flags[64, R - 1, C - 1] = BIT
	stamps = np.asarray([(18, 23, 60, 70), (0, 1, 0, 1), (R - 1, R, C - 1, C), (0, R, 0, C), (0, 1, 1, 2), (R - 1, R, C - 2, C - 1), (0, R, 1, C - 1)], dtype='int64')
	return flags, stamps


#: name -> changes to the arguments of a good call (T = 2 on the (5, 7) region, two stamps) that must be refused
REFUSALS = {
	'stamp_above': {'stamps': [(ROW0 - 1, ROW0 + 2, COL0, COL0 + 2)]},
	'stamp_below': {'stamps': [(ROW0 + 3, ROW0 + 6, COL0, COL0 + 2)]},
	'stamp_left': {'stamps': [(ROW0, ROW0 + 2, COL0 - 1, COL0 + 2)]},
	'stamp_right': {'stamps': [(ROW0, ROW0 + 2, COL0 + 5, COL0 + 8)]},
	'stamp_relative_not_ccd': {'stamps': [(0, 2, 0, 2)]},
	'stamp_rows_empty': {'stamps': [(ROW0 + 2, ROW0 + 2, COL0, COL0 + 2)]},
	'stamp_rows_reversed': {'stamps': [(ROW0 + 3, ROW0 + 2, COL0, COL0 + 2)]},
	'stamp_cols_empty': {'stamps': [(ROW0, ROW0 + 2, COL0 + 3, COL0 + 3)]},
	'stamp_partly_minus_one': {'stamps': [(-1, -1, -1, COL0 + 1)]},
	'second_stamp_bad': {'stamps': [(ROW0, ROW0 + 2, COL0, COL0 + 2), (ROW0, ROW0 + 6, COL0, COL0 + 2)]},
	'null_flags': {'null': 1},
	'null_stamps': {'null': 2},
	'null_out': {'null': 3},
	'flag_mask_zero': {'flag_mask': 0},
	'no_frames': {'n_frames': 0},
	'negative_frames': {'n_frames': -1},
	'no_targets': {'n_targets': 0},
	'pitch_below_frames': {'out_pitch': 1},
	'stride_below_frame': {'frame_stride': 34},
}


def refusal_base():
	flags = np.full((2, 5, 7), BIT, dtype='uint8')
	return {'flags': flags, 'n_frames': 2, 'frame_rows': 5, 'frame_cols': 7, 'frame_stride': 35, 'row0': ROW0, 'col0': COL0,
		'stamps': [(ROW0, ROW0 + 2, COL0, COL0 + 2), (ROW0 + 1, ROW0 + 5, COL0 + 3, COL0 + 7)], 'flag_mask': BIT, 'out_value': OUT_VALUE, 'out_pitch': 3, 'null': 0}
