# -*- coding: utf-8 -*-
"""
The launch rules of the stamp cutter (photometry_amd/csrc/cutout.hip, ``cut_stamps_launch``) restated without a device, and the case
table of tests/test_gpu_cutout_paths.py: one row per branch the launch code takes from a batch's geometry -- the per-stamp gather
with every carry pattern of its segment walk, with more than 64 KiB of dynamic LDS and at the documented width limit; the
frame-tile-major cut with stamps wider than a tile, frames of more than 1024 tiles, time pitches that are no multiple of anything;
stamps that miss the frame altogether on every path.  tests/test_cutout_cases_host.py holds the table to the classes it claims,
without a GPU.  The data and the expectation (``oracle.cutout.load_cube``, never the library) live here too.
"""
import numpy as np
import layout_common as lc

# the constants of cutout.hip the rules below depend on
CAD_BLOCK = 64                 # cutout.hip:37   kCadBlock: cadences per workgroup of the gather
MAX_STACKS = 4                 # cutout.hip:47   kMaxStacks
TILE_ROWS, TILE_COLS = 2, 64   # cutout.hip:130  kTileRows, kTileCols
TILE_CAD = 32                  # cutout.hip:131  kTileCad: frames per workgroup of the tile paths
SCAN_THREADS = 1024            # cutout.hip:171-175  tp_cut_scan_kernel: one workgroup, ceil(n_tiles / 1024) counts per thread
BAND_PIXELS = 64               # cutout.hip:385  rows per band: about 64 pixels
LDS_LIMIT = 160 * 1024         # cutout.hip:389  the TP_REQUIRE behind "wider than 639 pixels"
LDS_DEFAULT = 64 * 1024        # cutout.hip:449  above it the launch asks for the dynamic LDS with hipFuncSetAttribute
DENSE_FACTOR = 8               # cutout.hip:406, 427  stamps covering at least an eighth of the frame go tile by tile
SEG_LANES = 16                 # cutout.hip:71   lanes per row segment of the gather's load phase

N_EXTRA = 13                   # the stamps make_stamps adds to the random ones: 8 edges and corners, 4 wholly outside, 1 duplicate
EDGE = slice(-13, -5)
OUTSIDE = slice(-5, -1)
DUPLICATE = -1


def round_up(n, m):
	return (n + m - 1) // m * m


def launch_facts(T, R, C, H, W, n, t_pitch=None, masked=False):
	"""What ``cut_stamps_launch`` decides for ``n`` stamps of ``H x W`` on ``T`` frames of ``R x C`` (``n`` is the real stamp count)."""
	t_pitch = round_up(T, 32) if t_pitch is None else int(t_pitch)
	assert t_pitch >= T
	band_rows = min(max(BAND_PIXELS // W, 1), H)
	n_bands = (H + band_rows - 1) // band_rows
	shmem = CAD_BLOCK * ((band_rows * W) | 1) * 4
	dense = n * H * W * DENSE_FACTOR >= R * C
	if masked:
		path = 'tiles_pixels' if dense else 'gather'
	else:
		path = 'tiles' if dense else 'gather'
	n_tiles = ((C + TILE_COLS - 1) // TILE_COLS) * ((R + TILE_ROWS - 1) // TILE_ROWS)
	block = CAD_BLOCK if path == 'gather' else TILE_CAD
	cad_blocks = (t_pitch + block - 1) // block
	return dict(path=path, band_rows=band_rows, n_bands=n_bands, last_band_rows=H - (n_bands - 1) * band_rows,
		wgrp=(W + SEG_LANES - 1) // SEG_LANES, shmem=shmem, needs_attribute=shmem > LDS_DEFAULT, refused=shmem > LDS_LIMIT,
		n_tiles=n_tiles, scan_per=(n_tiles + SCAN_THREADS - 1) // SCAN_THREADS,
		t_pitch=t_pitch, cad_block=block, cad_blocks=cad_blocks, cad_blocks_beyond=sum(1 for b in range(cad_blocks) if b * block >= T))


def make_frames(T, R, C, seed):
	"""float32 ``(T, R, C)``: normal values with 2 % NaN (as ``layout_common.cut_frames``) and a sprinkle of +inf, -inf and -0.0 -- values
	that do not survive arithmetic, so that a bit-for-bit comparison catches a pixel that went through any."""
	rng = np.random.default_rng(seed)
	f = rng.standard_normal((T, R, C), dtype='float32')
	f[rng.random((T, R, C), dtype='float32') < 0.02] = np.nan
	flat = f.reshape(-1)
	k = max(4, flat.size // 200)
	pos = rng.integers(0, flat.size, 3 * k)
	flat[pos[:k]] = np.inf
	flat[pos[k:2 * k]] = -np.inf
	flat[pos[2 * k:]] = -0.0
	return f


def _origins(rng, size, extent, n):
	"""``n`` random first rows (columns) of stamps ``extent`` long on a frame ``size`` long, reaching up to three pixels over either
	edge; a stamp longer than the frame covers it and sticks out on both sides."""
	lo, hi = min(-3, size - extent - 3), max(size - extent + 3, -3)
	return rng.integers(lo, hi + 1, n)


def make_stamps(R, C, H, W, n, seed, row_offset=0, col_offset=lc.COL_OFFSET):
	"""int32 ``(n + 13, 4)`` stamps (row_min, row_max, col_min, col_max) in CCD coordinates: ``n`` random ones, the eight edge and
	corner stamps of ``layout_common.cut_stamps``, four that miss the frame altogether (above, below, left -- ending exactly at
	column 0 --, right) and a copy of stamp 0."""
	assert n >= 1
	rng = np.random.default_rng(seed)
	r0 = list(_origins(rng, R, H, n))
	c0 = list(_origins(rng, C, W, n))
	edge = [(-2, C // 2), (R - H + 2, C // 2), (R // 2, -2), (R // 2, C - W + 2), (-1, -1), (-1, C - W + 1), (R - H + 1, -1), (R - H + 1, C - W + 1)]
	outside = [(-H - 1, C // 3), (R, C // 2), (R // 2, -W), (R // 3, C + 5)]
	for (r, c) in edge + outside + [(r0[0], c0[0])]:
		r0.append(r)
		c0.append(c)
	r0 = np.array(r0, dtype='int64') + row_offset
	c0 = np.array(c0, dtype='int64') + col_offset
	return np.stack((r0, r0 + H, c0, c0 + W), axis=1).astype('int32')


def expected(frames, stamps, row_offset=0, col_offset=lc.COL_OFFSET):
	"""float32 ``(n, H, W, T)``: ``oracle.cutout.load_cube`` stamp by stamp."""
	from oracle import cutout
	return np.stack([cutout.load_cube(frames, tuple(int(v) for v in s), row_offset, col_offset) for s in stamps])


def _case(T, R, C, H, W, n, t_pitch=None, offsets=(0, lc.COL_OFFSET)):
	return dict(T=T, R=R, C=C, H=H, W=W, n=n, t_pitch=t_pitch, offsets=offsets)


# name -> T, R, C, H, W, n (the random stamps: make_stamps adds 13), t_pitch (None: round_up(T, 32)), (row_offset, col_offset).
# The prefix is the path the unmasked launch takes: g_ the per-stamp gather, t_ the frame-tile-major cut.  The gather needs the
# stamps (all n + 13) to cover less than an eighth of the frame, hence the larger frames under the larger stamps.
CASES = {
	# -- gather: wgrp = ceil(W / 16) segments per stamp row, advanced 16 at a time with a carry pattern of its own per 16 % wgrp
	'g_62x17': _case(33, 300, 400, 62, 17, 1),        # wgrp 2, band_rows 3, last band 2 rows (a shape of the resize loop)
	'g_5x32': _case(33, 200, 300, 5, 32, 10),         # wgrp 2, band_rows 2, last band 1 row
	'g_4x33': _case(33, 200, 300, 4, 33, 10),         # wgrp 3 (16 % 3 = 1: a carry every third step), band_rows 1
	'g_3x64': _case(33, 200, 300, 3, 64, 10),         # wgrp 4, band_rows 1
	'g_2x65': _case(33, 200, 300, 2, 65, 10),         # wgrp 5, bands of one row: di = 0, every carry bumps the cadence
	'g_3x100': _case(33, 200, 300, 3, 100, 6),        # wgrp 7 (16 % 7 = 2)
	'g_45x67': _case(70, 560, 610, 67, 45, 1),        # the bright-star default stamp; a second 64-cadence block, partly real
	'g_2x256': _case(33, 200, 300, 2, 256, 1),        # 65 792 B of LDS: the first size that takes the attribute branch
	'g_1x639': _case(33, 250, 300, 1, 639, 1),        # 163 584 B: the documented limit; wider than the frame
	'g_1x1': _case(33, 200, 300, 1, 1, 20),
	'g_pitch_odd': _case(37, 200, 300, 15, 15, 10, t_pitch=37),          # a pitch that is no multiple of 4 or 32
	'g_pitch_far': _case(33, 200, 300, 15, 15, 10, t_pitch=33 + 160),    # whole 64-blocks in the padding
	'g_offsets': _case(33, 200, 300, 11, 17, 10, offsets=(100, 44)),
	# the same carry patterns with every cadence of the 64-block real: at T = 33 the second half of the LDS tile is never stored, and a
	# walk that falls behind (a dropped carry) still happens to visit every segment of the first half
	'g_4x33_t64': _case(64, 200, 300, 4, 33, 10),
	'g_2x65_t64': _case(64, 200, 300, 2, 65, 10),
	'g_3x100_t64': _case(64, 200, 300, 3, 100, 6),
	# -- tile path
	't_9x70': _case(65, 31, 200, 9, 70, 4),           # a stamp spans 3 tile columns; odd last tile row, ragged last tile column
	't_3x130': _case(33, 20, 260, 3, 130, 4),         # spans 4 tile columns
	't_1x1': _case(33, 8, 64, 1, 1, 64),
	't_1cad': _case(1, 30, 30, 15, 15, 5),            # one frame
	't_scan_1024': _case(5, 128, 1024, 15, 15, 80),   # exactly 1024 tiles: one count per thread of the scan
	't_scan_1040': _case(5, 130, 1024, 15, 15, 80),   # 1040 tiles: two counts per thread, threads 520 .. 1023 idle
	't_scan_2210': _case(5, 260, 1030, 15, 15, 150),  # 17 x 130 tiles: three counts per thread, a last tile column 6 pixels wide
	't_pitch_odd': _case(37, 40, 60, 15, 15, 5, t_pitch=37),             # k_store / k_ok differ from lane to lane
	't_pitch_far': _case(33, 40, 60, 15, 15, 5, t_pitch=33 + 160),       # 32-blocks wholly in the padding
	't_offsets': _case(33, 50, 70, 11, 17, 20, offsets=(100, 44)),
}


def case_stamps(name):
	c = CASES[name]
	return make_stamps(c['R'], c['C'], c['H'], c['W'], c['n'], seed=c['T'] + c['W'], row_offset=c['offsets'][0], col_offset=c['offsets'][1])


def case_facts(name, masked=False):
	c = CASES[name]
	return launch_facts(c['T'], c['R'], c['C'], c['H'], c['W'], c['n'] + N_EXTRA, t_pitch=c['t_pitch'], masked=masked)


def case_masks(n, H, W):
	"""uint8 ``(n, H, W)``: the masks of test_gpu_frame_layouts.test_cut_stamps -- an empty one, a full one, 16 % random -- with 50 %
	more on the 13 stamps at the end (the ones that leave or miss the frame)."""
	rng = np.random.default_rng(23)
	mask = (rng.random((n, H, W)) < 0.16).astype('uint8')
	mask[0] = 0
	mask[1] = 1
	mask[-N_EXTRA:] |= (rng.random((N_EXTRA, H, W)) < 0.5).astype('uint8')
	return mask
