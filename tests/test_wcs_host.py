# -*- coding: utf-8 -*-
"""
CPU checks of the 'wcs' movement kernel: the header parser and its refusals (photometry_amd.wcs), the spherical-trigonometry
restatement tests/wcs_common.py against astropy's and the reference's own outputs (golden_wcs.npz, tests/golden/make_golden_wcs.py),
and the host side of MovementKernel('wcs') that needs no device.
"""
import os
import numpy as np
import pytest
from photometry_amd import wcs as W
from photometry_amd.motion import MovementKernel
import wcs_common as wc

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'golden_wcs.npz')


@pytest.fixture(scope='module')
def g():
	return dict(np.load(GOLDEN))


def _card(key, value):
	return f"{key:<8}= {value:>20}".ljust(80)


def _hdr(extra=(), drop=()):
	cards = [('WCSAXES', '2'), ('CTYPE1', "'RA---TAN-SIP'"), ('CTYPE2', "'DEC--TAN-SIP'"), ('CRPIX1', '1045.0'), ('CRPIX2', '1001.0'),
		('CRVAL1', '84.1'), ('CRVAL2', '-62.3'), ('CD1_1', '-0.0058'), ('CD1_2', '0.0001'), ('CD2_1', '0.0001'), ('CD2_2', '0.0058'),
		('A_ORDER', '2'), ('B_ORDER', '2'), ('A_2_0', '1.0D-6'), ('B_0_2', '-2.0E-6')]
	cards = [c for c in cards if c[0] not in drop] + list(extra)
	return ''.join(_card(k, v) for k, v in cards)


def test_parse_cards_forms():
	s = _hdr(extra=[('CTYPE1P', "'RAWX'"), ('WCSNAMEP', "'PHYSICAL'")]) + 'COMMENT   a comment'.ljust(80) + 'HISTORY x'.ljust(80) + ' ' * 80
	w = W.TanSipWCS.from_header(s)
	assert w.has_sip and w.a[0] == 2 and w.a[1][2, 0] == 1.0e-6 and w.b[1][0, 2] == -2.0e-6
	assert w.lonpole == 180.0 and np.array_equal(w.crval, [84.1, -62.3])
	# newline-separated cards and a dict give the same model
	w2 = W.TanSipWCS.from_header('\n'.join(s[i:i + 80].rstrip() for i in range(0, len(s), 80)))
	w3 = W.TanSipWCS.from_header({k: v for k, v in W.parse_cards(s).items()})
	for o in (w2, w3):
		np.testing.assert_array_equal(o.params(), w.params())
	assert W.parse_cards(_card('X', "'it''s'"))['X'] == "it's"


def test_sip_dmax_cards_are_ignored():
	"""A_DMAX / B_DMAX (the largest SIP distortion, present in TESS and other SIP headers) are read and ignored, as astropy does."""
	plain = W.TanSipWCS.from_header(_hdr())
	w = W.TanSipWCS.from_header(_hdr(extra=[('A_DMAX', '44.72893589844534'), ('B_DMAX', '4.462692873032506D+01')]))
	np.testing.assert_array_equal(w.params(), plain.params())


def test_pc_cdelt_and_no_sip():
	w = W.TanSipWCS.from_header(_hdr(extra=[('CDELT1', '-0.0058'), ('CDELT2', '0.0058'), ('PC1_1', '1.0'), ('PC2_2', '1.0')],
		drop=('CD1_1', 'CD1_2', 'CD2_1', 'CD2_2', 'A_ORDER', 'B_ORDER', 'A_2_0', 'B_0_2')))
	assert not w.has_sip
	np.testing.assert_array_equal(w.cd, [[-0.0058, 0.0], [0.0, 0.0058]])


@pytest.mark.parametrize('extra,drop,word', [
	([('CTYPE1', "'RA---SIN'")], ('CTYPE1',), 'CTYPE1'),
	([('PV2_1', '0.5')], (), 'PV2_1'),
	([('CPDIS1', "'Lookup'")], (), 'CPDIS1'),
	([('D2IMDIS1', "'Lookup'")], (), 'D2IMDIS1'),
	([('CTYPE3', "'WAVE'")], (), 'CTYPE3'),
	([('CD1_1', '0.0'), ('CD1_2', '0.0')], ('CD1_1', 'CD1_2'), 'CD'),
	([], ('B_ORDER',), 'B_ORDER'),
	([('A_ORDER', '10')], ('A_ORDER',), 'A_ORDER'),
])
def test_refusals_name_the_keyword(extra, drop, word):
	with pytest.raises(ValueError, match=word):
		W.TanSipWCS.from_header(_hdr(extra=extra, drop=drop))


def test_rotation_matrix_is_orthonormal():
	for crval, lp in (((84.1, -62.3), 180.0), ((0.0, 90.0), 0.0), ((359.9, 5.0), 170.0)):
		M = W.rotation_matrix(crval[0], crval[1], lp)
		np.testing.assert_allclose(M @ M.T, np.eye(3), atol=1e-15)
		# the native pole maps to CRVAL
		ra, dec = np.deg2rad(crval)
		np.testing.assert_allclose(M[:, 2], [np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)], atol=1e-15)


def test_restatement_against_astropy(g):
	for i, name in enumerate(g['hdr_names']):
		r = wc.RefWCS(str(g['hdr_strings'][i]))
		pts = g[f'hdr_{i}_pix']
		w = r.all_pix2world(pts, 0)
		assert wc.ra_diff(w[:, 0], g[f'hdr_{i}_all_pix2world'][:, 0]).max() < 1e-10, name
		assert np.abs(w[:, 1] - g[f'hdr_{i}_all_pix2world'][:, 1]).max() < 1e-10, name
		w1 = r.all_pix2world(pts, 1)
		assert wc.ra_diff(w1[:, 0], g[f'hdr_{i}_all_pix2world_o1'][:, 0]).max() < 1e-10, name
		assert wc.ra_diff(r.wcs_pix2world(pts, 0)[:, 0], g[f'hdr_{i}_wcs_pix2world'][:, 0]).max() < 1e-10, name
		assert np.abs(r.pix2foc(pts, 0) - g[f'hdr_{i}_pix2foc']).max() < 1e-10, name
		fp = r.all_pix2world(np.array([[0.0, 0.0], [0.0, 2077.0], [2135.0, 2077.0], [2135.0, 0.0]]), 0)
		assert wc.ra_diff(fp[:, 0], g[f'hdr_{i}_footprint'][:, 0]).max() < 1e-10, name
		# calc_footprint(axes=(2, 2)): the corners load_series' check sends back through all_world2pix (image_motion.py:300-309)
		fp22 = r.all_pix2world(np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.0]]), 0)
		assert wc.ra_diff(fp22[:, 0], g[f'hdr_{i}_footprint22'][:, 0]).max() < 1e-10, name
		assert np.abs(fp22[:, 1] - g[f'hdr_{i}_footprint22'][:, 1]).max() < 1e-10, name
		for b in (0, 1):
			world = g[f'hdr_{i}_world{b}']
			np.testing.assert_allclose(r.wcs_world2pix(world, 0), g[f'hdr_{i}_wcs_world2pix{b}'], rtol=0, atol=1e-8, err_msg=name)
			pix, k, div, slow = r.all_world2pix(world, 0)
			assert k == int(g[f'hdr_{i}_iters{b}']), (name, b, k)
			np.testing.assert_array_equal(div, g[f'hdr_{i}_divergent{b}'], err_msg=name)
			np.testing.assert_array_equal(slow, g[f'hdr_{i}_slow{b}'], err_msg=name)
			ok = ~div
			np.testing.assert_allclose(pix[ok], g[f'hdr_{i}_all_world2pix{b}'][ok], rtol=0, atol=1e-8, err_msg=name)
		assert r.corner_ok() == bool(g[f'hdr_{i}_corner_ok']), name
	assert not bool(g[f'hdr_{list(g["hdr_names"]).index("divergent")}_corner_ok'])    # the divergent header's corner
	# the SIP headers of the fixture carry A_DMAX / B_DMAX, as TESS headers do
	assert all('A_DMAX' in str(h) for n, h in zip(g['hdr_names'], g['hdr_strings']) if n != 'nosip')


def test_restatement_load_series(g):
	keep = [bool(h.strip()) and wc.RefWCS(str(h)).corner_ok() for h in g['series_headers']]
	np.testing.assert_array_equal(keep, g['series_kept'])
	assert 1 <= (~g['series_kept']).sum() <= 3


def test_wcs_needs_reference_to_be_used():
	"""Without wcs_ref the mode is refused where it is used, as before (test_motion_host.test_wcs_is_not_available)."""
	mk = MovementKernel(warpmode='wcs')
	with pytest.raises(NotImplementedError, match='astropy.wcs'):
		mk.jitter(np.array([1.0]), 1.0, 2.0)
	with pytest.raises(NotImplementedError, match='astropy.wcs'):
		MovementKernel(warpmode='affine', wcs_ref=_hdr())


def test_wcs_load_series_length_check():
	mk = MovementKernel(warpmode='wcs', wcs_ref=_hdr())
	assert isinstance(mk.wcs_ref, W.TanSipWCS)
	with pytest.raises(ValueError, match='Wrong shape of kernels'):
		mk.load_series(np.arange(3.0), [_hdr(), _hdr()])
	with pytest.raises(ValueError, match='Interpolator is not defined'):
		mk.interpolate(1.0, [[1.0, 2.0]])


def test_frame_pairs_follow_interpolate(g):
	"""The (k1, k2, dt, dx) rule of image_motion.py:357-389, without the device."""
	mk = MovementKernel(warpmode='wcs', wcs_ref=_hdr())
	st = np.array([1.0, 2.0, 3.0, 5.0])
	mk.series_times = st
	k1, k2, dt, dx = mk._wcs_frame_pairs(np.array([1.0, 2.5, 5.0, 0.2, 5.9, 3.0, 4.5]))
	np.testing.assert_array_equal(k1, [0, 1, 3, 0, 3, 2, 2])
	np.testing.assert_array_equal(k2, [-1, 2, -1, -1, -1, -1, 3])
	np.testing.assert_array_equal(dx[[1, 6]], [0.5, 1.5])
	np.testing.assert_array_equal(dt[[1, 6]], [1.0, 2.0])
	for bad in (-0.01, 6.01, np.nan):
		with pytest.raises(ValueError, match='outside'):
			mk._wcs_frame_pairs(np.array([bad]))
