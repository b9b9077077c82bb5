# -*- coding: utf-8 -*-
"""
The mask + extraction launch (``tp_aperture_fused_kernel<VEC, VEC4, HAS_SUB, BKG, A1>``, csrc/fused.hip) in every one of its 24
instantiations, its streamed extraction (``extract_small_stream``, csrc/aperture_dev.h) in both of its forms -- the series staged in
LDS, or re-read from HBM with every pixel group where they do not fit -- and the kernel of the masks above 128 pixels
(``tp_aperture_big_kernel``) in the series, subtract and no-background modes: against ``oracle/aperture.py`` (the float32 sums bit
for bit, the float64 centroids to 1e-12 relative with the same NaN pattern -- the tolerance of tests/test_gpu_aperture.py) and
against the stand-alone entries ``tp_sumimage`` + ``tp_k2p2_masks`` + ``tp_aperture_extract``, byte for byte.

Which form of the streamed extraction a target takes is decided by ``need <= room`` (extract_variants_common.py restates the rule and
tests/test_extract_variants_host.py holds it to the kernel's layout function and shows that the cadence counts below lie on both
sides of it).  Throughout, the padding of every input series and cube is NaN and the light-curve arrays have a pitch above the
cadence count and are prefilled with a byte pattern: no result may depend on the one, the other must come back intact.
"""
import numpy as np
import pytest
import extract_variants_common as evc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _check_against_oracle(b, got, ref, T, name):
	for i in range(b.n):
		tag = f"{name} target {i} M={int(b.mask(i).sum())}"
		# (the status of the 2^30 target: see tests/test_gpu_extract_loop.py)
		if b.stamps[i].max() < 2**24:
			assert int(got['status'][i]) == b.ref[i]['status'], tag
		np.testing.assert_array_equal(got['mask'][i].astype(bool), b.mask(i), err_msg=tag)
		evc.check_lightcurve(got, i, ref[i], T, tag)
	evc.check_padding(got, T, tag=name)


# ---- both forms of the streamed extraction, at the seam ------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,T,mode", evc.seam_cases())
def test_streamed_extraction_at_the_seam(ctx, H, W, T, mode):
	"""Masks of 1 .. 128 pixels, cadence counts R - 1 .. R + 2 around every room R (around R / 2 where two series are staged), with
	aligned pitches (VEC 2) and with pitches that force the scalar kernels (VEC 1)."""
	b = evc.seam_batch(H, W)
	d = evc.seam_cubes(b, T, mode)
	ref = evc.reference(b, d)
	scene = evc.meta_scene(b, T)
	ns = evc.n_series(mode)
	for aligned in (True, False):
		forms = {evc.staged(H, W, M, T, evc.vec_of(aligned), ns) for M in evc.mask_sizes(b)}
		inp = evc.Inputs(ctx, d, aligned)
		fused = evc.run(ctx, scene, inp, b.sumimage, 'fused')
		alone = evc.run(ctx, scene, inp, b.sumimage, 'alone')
		name = f"{mode} T={T} {'aligned' if aligned else 'unaligned'} (LDS-staged forms among the targets: {sorted(forms)})"
		_check_against_oracle(b, fused, ref, T, "fused, " + name)
		_check_against_oracle(b, alone, ref, T, "stand-alone, " + name)
		evc.check_same_bytes(fused, alone, evc.LC_COLUMNS + ('mask',), name)


# ---- every instantiation ---------------------------------------------------------------------------------------------------------------

_SUMIMAGES = {}


def _device_sumimage(ctx, shape, inp, subtract, aligned):
	"""tp_sumimage of the scene's images minus the subtracted series: what a caller that has the sum image hands to the launch."""
	from photometry_amd import engine
	key = (shape, subtract, aligned)
	if key not in _SUMIMAGES:
		s = evc.raw_scene(shape)
		S = engine.sumimage(ctx, inp.img, ctx.array(np.asarray(s.quality, dtype='int32')), subtract=inp.sub).to_host()
		ctx.sync()
		_SUMIMAGES[key] = S
	return _SUMIMAGES[key]


@pytest.mark.parametrize("pair", evc.PAIRS, ids=lambda p: p[0] + '+' + p[1])
@pytest.mark.parametrize("given", [False, True], ids=['a1', 'given'])
@pytest.mark.parametrize("aligned", [True, False], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize("name", sorted(evc.SCENES))
def test_every_instantiation(ctx, name, aligned, given, pair):
	"""(VEC, VEC4) x HAS_SUB x BKG x A1: 28 runs per scene, all 24 instantiations; the stand-alone entries with the same arguments; the
	oracle fed the device's sum image (so that no threshold razor enters)."""
	from oracle import aperture as oap, sumimage as osum
	shape = evc.SCENES[name]
	s = evc.raw_scene(shape)
	Nt, T, H, W = s.n_targets, s.n_cad, s.height, s.width
	d = evc.scene_inputs(shape, pair)
	inp = evc.Inputs(ctx, d, aligned)
	S_in = _device_sumimage(ctx, shape, inp, pair[0], aligned) if given else None
	fused = evc.run(ctx, s, inp, S_in, 'fused')
	alone = evc.run(ctx, s, inp, S_in, 'alone')
	tag = f"{name} {'aligned' if aligned else 'unaligned'} {'given' if given else 'a1'} {pair}"
	# the other side: every key, bit for bit
	assert (alone['status'] != 2).any(), tag
	evc.check_same_bytes(fused, alone, evc.KEYS, tag)
	# the sum image of raw - series
	img = d['raw'] if d['sub'] is None else (d['raw'] - d['sub'][:, None, None, :]).astype('float32')
	S_ref = osum.sumimage_batch(img, s.quality)
	np.testing.assert_array_equal(np.isnan(fused['sumimage']), np.isnan(S_ref), err_msg=tag)
	np.testing.assert_allclose(fused['sumimage'], S_ref, rtol=1e-12, atol=0, equal_nan=True, err_msg=tag)
	# the light curves, from the device's sum image
	n_ok = 0
	rows = []
	for i in range(Nt):
		if d['cube'] is not None:
			bkg = d['cube'][i]
		else:
			bkg = None if d['ser'] is None else np.broadcast_to(d['ser'][i][None, None, :], img[i].shape)
		try:
			ref = oap.do_photometry(fused['sumimage'][i], img[i], d['err'][i], bkg, tuple(s.stamps[i]), s.target_pos_row[i], s.target_pos_column[i],
				s.target_tmag[i], s.target_starid[i], s.catalog_of(i), np.ones((H, W), dtype='int32'))
		except Exception as e: # noqa: B902 -- any exception of the plugin is STATUS.ERROR
			ref = {'status': oap.STATUS_ERROR, 'exception': repr(e)}
		assert int(fused['status'][i]) == ref['status'], (tag, i, ref.get('errors'), ref.get('exception'))
		if ref['status'] == oap.STATUS_ERROR or ref.get('mask') is None:
			continue
		np.testing.assert_array_equal(fused['mask'][i].astype(bool), ref['mask'], err_msg=f"{tag} target {i}")
		evc.check_lightcurve(fused, i, ref, T, f"{tag} target {i}")
		if pair[1] == 'none':
			assert np.isnan(fused['flux_background'][i, :T]).all()
		rows.append(i)
		n_ok += 1
	assert n_ok >= 1, tag
	evc.check_padding(fused, T, rows=rows, tag=tag)


# ---- masks above 128 pixels in the series modes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize("mode", evc.BIG_MODES)
@pytest.mark.parametrize("T", evc.BIG_T)
def test_big_masks_in_series_modes(ctx, T, mode, aligned):
	"""The fused launch hands the masks above 128 pixels to tp_aperture_big_kernel through its work list; tp_aperture_extract finds them
	itself: both against the oracle and each other."""
	b = evc.big_batch()
	d = evc.big_cubes(b, T, mode)
	ref = evc.reference(b, d)
	scene = evc.meta_scene(b, T)
	inp = evc.Inputs(ctx, d, aligned)
	name = f"{mode} T={T} {'aligned' if aligned else 'unaligned'}"
	fused = evc.run(ctx, scene, inp, b.sumimage, 'fused')
	_check_against_oracle(b, fused, ref, T, "fused, " + name)
	direct = evc.extract_with_mask(ctx, scene, inp, np.stack([b.mask(i) for i in range(b.n)]))
	for i in range(b.n):
		evc.check_lightcurve(direct, i, ref[i], T, f"tp_aperture_extract, {name} target {i} M={int(b.mask(i).sum())}")
	evc.check_padding(direct, T, tag=name)
	evc.check_same_bytes(fused, direct, evc.LC_COLUMNS, name)


# ---- the shapes real data has ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(evc.LONG_SCENES))
def test_raw_step_on_long_series(ctx, name):
	"""pipeline.aperture_step on raw cubes whose series do not fit the LDS (every target takes the HBM-series form: asserted with
	staged() here and in the CPU file) against the oracle-only chain of tests/test_gpu_raw_chain.py."""
	from photometry_amd import pipeline
	from oracle import aperture as oap, k2p2 as ok2p2
	shape = evc.LONG_SCENES[name]
	s = evc.raw_scene(shape)
	Nt, T, H, W = s.n_targets, s.n_cad, s.height, s.width
	orc = evc.oracle_chain(shape)
	batch = pipeline.ApertureBatch(ctx, s, cubes='host_raw')
	assert batch.time_smooth == evc.TIME_SMOOTH
	work = pipeline.ApertureWork(ctx, batch)
	pipeline.aperture_step(ctx, batch, work)
	ctx.sync()
	got = work.lc.to_host()
	got.update(bkg_raw=work.bkg_raw.to_host()[:, :T], bkg=work.bkg.to_host()[:, :T], S=work.sumimage.to_host().reshape(Nt, H, W),
		mask=work.mask.to_host().reshape(Nt, H, W), status=work.status.to_host())
	n_exact = n_razor = 0
	for i, o in enumerate(orc):
		np.testing.assert_array_equal(got['bkg_raw'][i], o['bkg_raw'], err_msg=f"B* of target {i}")
		np.testing.assert_array_equal(got['bkg'][i], o['bkg'], err_msg=f"B2 of target {i}")
		np.testing.assert_allclose(got['S'][i], o['S'], rtol=1e-12, atol=0, equal_nan=True)
		ref = o['ref']
		same = int(got['status'][i]) == ref['status'] and (ref['mask'] is None or np.array_equal(got['mask'][i].astype(bool), ref['mask']))
		if not same:
			# a sum-image pixel within rounding of K2P2's threshold: allowed exactly as tests/test_gpu_raw_chain.py allows it
			thr = ok2p2.threshold(o['S'], 0.8, full_output=True)
			with np.errstate(invalid='ignore'):
				margin = np.nanmin(np.abs(o['S'] - thr['CUT']))
			assert margin <= 8e-6 * max(1.0, abs(thr['CUT'])), f"target {i}: masks differ off the razor's edge (margin {margin}, CUT {thr['CUT']}, status {got['status'][i]} vs {ref['status']})"
			n_razor += 1
			continue
		assert ref['status'] != oap.STATUS_ERROR and ref['mask'] is not None, i
		M = int(ref['mask'].sum())
		assert M <= 128 and not evc.staged(H, W, M, T, 2, 1), (i, M)
		evc.check_lightcurve(got, i, ref, T, f"{name} target {i} M={M}")
		n_exact += 1
	assert n_razor == 0, "a razor case on the committed seed"
	assert n_exact == Nt
