# -*- coding: utf-8 -*-
"""
``photometry_amd.tpf`` on the device: ``load_tpfs`` on small target pixel files written by tests/tpf_common.py (not by
``photometry_amd.fitsio``), held bit for bit to numpy's reading of the same records, and a ``datasource='tpf'`` run of the aperture
plugin on a ``TpfStampSource`` held bit for bit to the same class on a ``MemoryStampSource`` with the identical numpy inputs.
"""
import numpy as np
import pytest
import ffi_common as fc
import tpf_common as tc
from alloc_common import count_allocations
from photometry_amd import ffi, tpf

pytestmark = pytest.mark.gpu

NAMES = ['tess2019199201929-s0014-%016d-0150-s_tp.fits' % n for n in (11, 22, 33)]


@pytest.fixture(scope='module')
def ctx():
	from photometry_amd.device import Context
	c = Context(0)
	yield c
	c.close()


def _same_bits(a, b):
	a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
	return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view('uint8'), b.view('uint8'))


# ---- three files in one call --------------------------------------------------------------------------------------------------------
BAD = (0, 17, 18, 69)


@pytest.fixture(scope='module')
def three(tmp_path_factory):
	"""11 x 11 x 70; 9 x 13 x 40 as .gz without the READNOIA / GAINA / NUM_FRM / NREADOUT cards; 11 x 11 x 70 with four non-finite TIMEs."""
	root = tmp_path_factory.mktemp('tpf')
	rng = np.random.default_rng(77)
	made = [tc.make_tpf(rng, 11, 11, 70, crval1p=200, crval2p=300),
		tc.make_tpf(rng, 9, 13, 40, table_extra=[], crval1p=1045, crval2p=7, primary=dict(SECTOR=15, CAMERA=4, CCD=1, DATA_REL=36)),
		tc.make_tpf(rng, 11, 11, 70, bad_times=BAD, crval1p=44 + 1, crval2p=1)]
	files = [fc.write(root / (NAMES[k] + ('.gz' if k == 1 else '')), made[k][0]) for k in range(3)]
	return {'files': files, 'made': made}


@pytest.fixture(scope='module')
def loaded3(ctx, three):
	order = [2, 0, 1]
	return order, tpf.load_tpfs(ctx, [three['files'][k] for k in order])


def test_cubes_are_numpys_reading_in_the_order_given(three, loaded3):
	order, loaded = loaded3
	assert [ld.path for ld in loaded] == [three['files'][k] for k in order]
	for ld, k in zip(loaded, order):
		blob, rec, ap, info = three['made'][k]
		good = np.isfinite(rec['TIME'])
		for name, col in (('images', 'FLUX'), ('images_err', 'FLUX_ERR'), ('backgrounds', 'FLUX_BKG')):
			cube = ld.cubes[name]
			H, W = ap.shape
			assert (cube.n_targets, cube.n_cad, cube.height, cube.width) == (1, int(good.sum()), H, W) and cube.t_pitch % 32 == 0
			want = tc.host_cube(rec, col, good)                       # (H, W, T) as uint32
			full = cube.data.to_host()
			assert full.dtype == np.float32 and np.array_equal(full[0, :, :, :cube.n_cad].view('uint32'), want), (k, name)
			assert np.all(full[0, :, :, cube.n_cad:].view('uint32') == 0)                       # the pads read 0.0 without a memset
			assert np.array_equal(cube.to_host()[0].view('uint32'), want)


def test_vectors_and_header_derived_attributes(three, loaded3):
	order, loaded = loaded3
	for ld, k in zip(loaded, order):
		blob, rec, ap, info = three['made'][k]
		good = np.isfinite(rec['TIME'])
		assert ld.rows_dropped == (4 if k == 2 else 0) == int((~good).sum())
		T = int(good.sum())
		assert _same_bits(ld.time, rec['TIME'][good].astype('float64')) and ld.time.dtype == np.float64          # DATA_REL 35 / 36: no offset
		assert ld.time_offset_corrected is False
		assert _same_bits(ld.timecorr, rec['TIMECORR'][good].astype('float32')) and ld.timecorr.dtype == np.float32
		assert _same_bits(ld.cadenceno, rec['CADENCENO'][good].astype('int32')) and _same_bits(ld.quality, rec['QUALITY'][good].astype('int32'))
		assert ld.pos_corr.shape == (T, 2) and ld.pos_corr.dtype == np.float64
		assert _same_bits(ld.pos_corr, np.column_stack((rec['POS_CORR1'][good], rec['POS_CORR2'][good])).astype('float64'))
		assert _same_bits(ld.aperture, ap) and ld.aperture.dtype == np.int32
		H, W = ap.shape
		c1p, c2p = ((200, 300), (1045, 7), (45, 1))[k]
		assert ld.max_stamp == (c2p - 1, c2p - 1 + H, c1p - 1, c1p - 1 + W)                                      # BasePhotometry.py:354-359
		want_primary = dict(tc.PRIMARY, **(dict(SECTOR=15, CAMERA=4, CCD=1, DATA_REL=36) if k == 1 else {}))
		assert (ld.sector, ld.camera, ld.ccd, ld.data_rel) == tuple(want_primary[key] for key in ('SECTOR', 'CAMERA', 'CCD', 'DATA_REL'))
		assert ld.header['PROCVER'] == 'spoc-5.0.20-20201120' and ld.header['TELESCOP'] == 'TESS' and ld.header['TICID'] == 261136679
		assert ld.cadence == 120
		if k == 1:
			assert (ld.readnoise, ld.gain, ld.num_frm, ld.n_readout) == (10, 100, 60, 48)                          # the reference's defaults
		else:
			assert (ld.readnoise, ld.gain, ld.num_frm, ld.n_readout) == (7.5, 5.25, 60, 48)
		assert 'CTYPE1' in ld.wcs_cards and 'CRVAL1P' not in ld.wcs_cards and len(ld.wcs_cards) % 80 == 0
		assert ld.stats['bytes'] == info['aperture_offset'] + info['aperture_bytes'] - info['table_offset'] and ld.stats['read_s'] > 0


def test_a_flipped_byte_outside_the_unpacked_columns(ctx, three, tmp_path, monkeypatch):
	blob, rec, ap, info = three['made'][0]
	at = info['table_offset'] + 5 * info['row_bytes'] + info['columns']['RAW_CNTS'] + 7                       # inside RAW_CNTS of row 5
	bad = bytearray(blob)
	bad[at] ^= 0x10
	path = fc.write(tmp_path / 'flipped_tp.fits', bytes(bad))
	live = count_allocations(ctx, monkeypatch)                                # every allocation and release on ctx, device and page-locked
	with pytest.raises(ffi.ChecksumError, match=r'flipped_tp\.fits: HDU 1'):
		tpf.load_tpfs(ctx, [three['files'][1], path], verify=True)
	assert live == {'device': 0, 'host': 0}, live
	(ld,) = tpf.load_tpfs(ctx, [path], verify=False)
	assert live == {'device': 3, 'host': 0}, live                             # the counter counts: the three cubes of the file
	assert np.array_equal(ld.cubes['images'].to_host()[0].view('uint32'), tc.host_cube(rec, 'FLUX'))
	ld.free()
	assert all(c is None for c in ld.cubes.values())
	assert live == {'device': 0, 'host': 0}, live


def test_a_double_image_column_is_refused_before_any_allocation(ctx, three, tmp_path, monkeypatch):
	blob, *_ = tc.make_tpf(np.random.default_rng(3), 5, 5, 8, image_code='>f8', image_letter='D')
	path = fc.write(tmp_path / 'double_tp.fits', blob)
	from photometry_amd import device
	def refuse(*args, **kwargs):
		raise AssertionError('allocated')
	monkeypatch.setattr(device.DeviceArray, '__init__', refuse)
	monkeypatch.setattr(device.PinnedArray, '__init__', refuse)
	with pytest.raises(ValueError, match=r"double_tp\.fits: image column FLUX has the TFORM '25D'"):
		tpf.load_tpfs(ctx, [three['files'][0], path])


def test_time_offset_applied_for_data_rel_20_not_for_35(ctx, tmp_path):
	rng = np.random.default_rng(8)
	files, recs = [], []
	for rel in (20, 35):
		blob, rec, ap, info = tc.make_tpf(rng, 5, 6, 33, bad_times=(4,), primary=dict(DATA_REL=rel, PROCVER='spoc-4.0.5-20190101'))
		files.append(fc.write(tmp_path / f'rel{rel}_tp.fits', blob))
		recs.append(rec)
	early, late = tpf.load_tpfs(ctx, files)
	good = np.isfinite(recs[0]['TIME'])
	assert early.time_offset_corrected is True and late.time_offset_corrected is False
	assert _same_bits(early.time, recs[0]['TIME'][good].astype('float64') + (-2.000 + 0.021) / 86400)            # fixes/time_offset.py:166
	assert _same_bits(late.time, recs[1]['TIME'][np.isfinite(recs[1]['TIME'])].astype('float64'))
	assert early.rows_dropped == late.rows_dropped == 1 and early.cubes['images'].n_cad == 32
	src = tpf.TpfStampSource(early, {'starid': np.array([5]), 'tmag': np.array([10.0]), 'row': np.array([301.0]), 'column': np.array([202.0])})
	assert src.header['TIME_OFFSET_CORRECTED'] is True and src.header['DATA_REL'] == 20 and src.time_offset_corrected
	assert tpf.TpfStampSource(late, src.catalog).header['TIME_OFFSET_CORRECTED'] is False
	for ld in (early, late):
		ld.free()


def test_a_catalogue_in_ra_dec_is_projected_through_the_aperture_wcs(loaded3):
	"""BasePhotometry.py:1159-1165, :461-464: the WCS of the APERTURE header is relative to the stamp; the stamp's place on the CCD is added."""
	from photometry_amd.wcs import as_wcs
	order, loaded = loaded3
	ld = loaded[1]
	w = as_wcs(ld.wcs_cards, ctx=ld.cubes['images'].ctx)
	radec = w.all_pix2world(np.array([[5.0, 5.0], [2.25, 7.25], [9.0, 1.0]]), 0)
	src = tpf.TpfStampSource(ld, {'starid': np.array([1, 2, 3]), 'tmag': np.array([9.0, 10.0, 11.0]), 'ra': radec[:, 0], 'dec': radec[:, 1]},
		targets={'starid': np.array([2]), 'tmag': np.array([10.0]), 'ra': radec[1:2, 0], 'dec': radec[1:2, 1]})
	px = w.all_world2pix(radec, 0)
	r0, _, c0, _ = ld.max_stamp
	assert (r0, c0) == (299, 199)
	assert _same_bits(src.catalog['column'], (px[:, 0] + c0).astype('float32')) and _same_bits(src.catalog['row'], (px[:, 1] + r0).astype('float32'))
	assert np.array_equal(np.round(src.catalog['column']), [204, 201, 208]) and np.array_equal(np.round(src.catalog['row']), [304, 306, 300])
	t = src.target(2)
	one = w.all_world2pix(radec[1:2], 0)[0]
	assert t['column'] == one[0] + c0 and t['row'] == one[1] + r0 and t['tmag'] == 10.0
	# pixel positions given: left as they are, and no WCS is built
	plain = tpf.TpfStampSource(ld, {'starid': np.array([1]), 'tmag': np.array([9.0]), 'row': np.array([301.5]), 'column': np.array([202.5])})
	assert plain.wcs is None and plain.catalog['row'][0] == 301.5
	assert plain.max_stamp == ld.max_stamp and plain.aperture_image is ld.aperture and plain.jitter is not None and plain.n_readout == 48 and plain.num_frm == 60


# ---- end to end through the plugin ----------------------------------------------------------------------------------------------
def _bits_equal(a, b):
	a, b = np.asarray(a), np.asarray(b)
	return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view('uint8'), np.ascontiguousarray(b).view('uint8'))


def test_aperture_plugin_on_a_tpf_equals_the_memory_source(ctx, tmp_path):
	from photometry_amd import simulate
	from photometry_amd.device import Context
	from photometry_amd.plugins import AperturePhotometry
	from photometry_amd.source import MemoryStampSource
	from photometry_amd.status import STATUS
	H = W = 11
	T = 70
	s = simulate.make_scene(2, T, H, W, seed=12, cadence_s=120.0)
	simulate.fill_cubes(s, nan_fraction=0.0)
	i = 0
	st = tuple(int(v) for v in s.stamps[i])
	rng = np.random.default_rng(5)
	cubes = {'FLUX': np.moveaxis(s.images[i], 2, 0).copy(), 'FLUX_ERR': np.moveaxis(s.images_err[i], 2, 0).copy(), 'FLUX_BKG': np.moveaxis(s.backgrounds[i], 2, 0).copy()}
	# APERTURE: 1 everywhere plus SPOC's mask (2) and centroid (8) bits and a channel bit on some pixels; two pixels never collected: NaN flux
	ap = np.ones((H, W), dtype='int32')
	ap[3:8, 3:8] |= 2
	ap[4:7, 4:7] |= 8
	ap[:, :6] |= 32
	ap[:, 6:] |= 64
	for r, c in ((0, 0), (H - 1, W - 1)):
		ap[r, c] &= ~1
		cubes['FLUX'][:, r, c] = np.nan
		cubes['FLUX_ERR'][:, r, c] = np.nan
	# the scene's own time base and jitter in the file's types
	scalars = {'TIME': s.time, 'TIMECORR': np.asarray(s.timecorr, dtype='float32'), 'QUALITY': s.quality, 'POS_CORR1': s.jitter[:, 0].astype('float32'),
		'POS_CORR2': s.jitter[:, 1].astype('float32')}
	blob, rec, ap_file, info = tc.make_tpf(rng, H, W, T, crval1p=st[2] + 1, crval2p=st[0] + 1, aperture=ap, images=cubes, scalars=scalars)
	path = fc.write(tmp_path / NAMES[0], blob)
	cat = s.catalog_of(i)
	catalog = {k: cat[k] for k in ('starid', 'tmag', 'row', 'column')}
	targets = {'starid': s.target_starid[i:i + 1], 'tmag': s.target_tmag[i:i + 1], 'row': s.target_pos_row[i:i + 1], 'column': s.target_pos_column[i:i + 1]}
	starid = int(s.target_starid[i])

	# the same inputs as numpy arrays, read by numpy from the records
	frames = {'images': np.moveaxis(rec['FLUX'].astype('uint32').view('float32'), 0, 2), 'images_err': np.moveaxis(rec['FLUX_ERR'].astype('uint32').view('float32'), 0, 2),
		'backgrounds': np.moveaxis(rec['FLUX_BKG'].astype('uint32').view('float32'), 0, 2)}
	jitter = np.column_stack((rec['POS_CORR1'], rec['POS_CORR2'])).astype('float64')
	mem = MemoryStampSource(frames, st[0], st[2], rec['TIME'].astype('float64'), rec['TIMECORR'].astype('float32'), rec['CADENCENO'].astype('int32'),
		rec['QUALITY'].astype('int32'), catalog, sector=14, camera=2, ccd=3, cadence=120, n_readout=48, jitter=jitter, targets=targets)
	mem.header = {'DATA_REL': 35}

	def run(source):
		with AperturePhotometry(starid, source, str(tmp_path), datasource='tpf', ctx=ctx) as pho:
			assert pho.stamp == st                                                  # the whole postage stamp (BasePhotometry.py:616-693)
			used = pho._device_cubes() is not None
			pho.photometry()
			return pho, used, np.array(pho.aperture), np.array(pho.sumimage)

	(loaded,) = tpf.load_tpfs(ctx, [path])
	want_pho, used, _, want_sum = run(mem)
	assert not used and want_pho.status in (STATUS.OK, STATUS.WARNING)
	got_pho, used, aperture, got_sum = run(tpf.TpfStampSource(loaded, catalog, targets=targets))
	assert used                                                                  # the loader's cubes went to the kernels as they are
	# on another context the cubes are cut out on the host: the same results
	other = Context(0)
	try:
		(loaded2,) = tpf.load_tpfs(other, [path])
		host_pho, used2, aperture2, host_sum = run(tpf.TpfStampSource(loaded2, catalog, targets=targets))
		assert not used2
		loaded2.free()
	finally:
		other.close()
	for pho, sumimage in ((got_pho, got_sum), (host_pho, host_sum)):
		assert pho.status == want_pho.status
		assert list(pho.lightcurve.keys()) == list(want_pho.lightcurve.keys())
		for key in pho.lightcurve.keys():
			assert _bits_equal(pho.lightcurve[key], want_pho.lightcurve[key]), key
		assert _bits_equal(pho.lightcurve['pos_corr'], jitter)
		assert _bits_equal(pho.final_phot_mask, want_pho.final_phot_mask) and _bits_equal(sumimage, want_sum)
		assert pho._details.get('stamp') == want_pho._details.get('stamp')
	assert np.isnan(got_sum[0, 0]) and np.isnan(got_sum[H - 1, W - 1]) and np.isfinite(got_sum).sum() == H * W - 2
	# the aperture of the file without the flags of SPOC's mask and centroid pixels, the rest intact (BasePhotometry.py:1063-1072)
	for a in (aperture, aperture2):
		assert a.dtype == np.int32 and np.array_equal(a, ap & ~(2 | 8)) and not np.any(a & (2 | 8))
		assert np.array_equal(a & 1, ap & 1) and np.array_equal(a & (32 | 64), ap & (32 | 64)) and a[0, 0] & 1 == 0 and np.any(ap & 2) and np.any(ap & 8)
	# the public entry: tessphot('aperture', starid, source, output, datasource='tpf') writes its light curve and returns the same
	from photometry_amd import tessphot
	out_dir = tmp_path / 'out'
	pho = tessphot('aperture', starid, tpf.TpfStampSource(loaded, catalog, targets=targets), str(out_dir), datasource='tpf', ctx=ctx)
	assert pho.status == want_pho.status and pho.datasource == 'tpf', pho._details
	for key in ('flux', 'flux_err', 'flux_background', 'pos_centroid', 'pos_corr', 'time'):
		assert _bits_equal(pho.lightcurve[key], want_pho.lightcurve[key]), key
	# the cubes the kernels were handed are as the loader left them
	assert np.array_equal(loaded.cubes['images'].to_host()[0].view('uint32'), frames['images'].view('uint32'))
	loaded.free()
