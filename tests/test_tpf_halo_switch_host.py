# -*- coding: utf-8 -*-
"""
The six target pixel files of tests/test_gpu_tpf_halo_switch.py (tests/halo_cubes_common.py) held to their conditions without a GPU:
the oracle's aperture photometry of every file on its fixed stamp, the edge flux of its mask, the switch predicate, and the Halo
problems of the switching files from the host restatement.
"""
import numpy as np
import halo_common as hc
import halo_cubes_common as cc


def test_the_files_meet_their_conditions_on_the_oracle():
	from oracle import aperture as oap, sumimage as osum, diagnostics as odiag
	from photometry_amd import halo
	tmag_limit, flux_limit = 6.0, 0.01
	spec = cc.switch_scenes()
	assert len(spec) == len(cc.FILES)
	shapes = [(s.height, s.width) for s, _, _, _, _ in spec]
	assert shapes.count((11, 11)) == 4 and shapes.count((9, 13)) == 2
	switching, n_seg = [], {}
	for f, (s, i, off, time, quality) in enumerate(spec):
		cubes, ap, time, quality = cc.file_arrays(s, i, time, quality)
		images, err, bkg = (np.ascontiguousarray(np.moveaxis(cubes[k], 0, 2)) for k in ('FLUX', 'FLUX_ERR', 'FLUX_BKG'))
		stamp = tuple(int(v) for v in s.stamps[i])
		tmag = float(s.target_tmag[i])
		sumimage = osum.sumimage(images, quality)
		o = oap.do_photometry(sumimage, images, err, bkg, stamp, float(s.target_pos_row[i]), float(s.target_pos_column[i]), tmag, int(s.target_starid[i]),
			s.catalog_of(i), ap & ~np.int32(2 | 8), datasource='tpf')
		assert o['status'] in (1, 3) and 'mask' in o, (cc.FILES[f], o['status'], o['errors'])
		d = odiag.diagnostics(time, quality, o['flux'], o['flux_err'], o['pos_centroid'], sumimage=sumimage, mask=o['mask'])
		assert d['flags'] & 7 == 0, (cc.FILES[f], d['flags'])
		ratio = d['edge_flux'] / hc.mag2flux(tmag)
		print(f"{cc.FILES[f]}: Tmag {tmag:.2f}, mask of {int(o['mask'].sum())} pixels, edge flux / expected flux {ratio:.4f}")
		if tmag <= tmag_limit and ratio > flux_limit:
			switching.append(f)
			assert ratio > 2 * flux_limit, 'the edge-flux reason should not hang on the last digits'
		elif tmag <= tmag_limit:
			assert ratio < 0.5 * flux_limit
		# the Halo problems of the file, every one of them (tessphot('halo') runs them all)
		seg = halo.segments(time, halo.split_times(14, time, np.full(len(time), 3e-3)))
		n_seg[f] = int(seg.max()) + 1
		mask = hc.pixel_mask(ap & ~np.int32(2 | 8), stamp, float(s.target_pos_row[i]), float(s.target_pos_column[i]))
		assert not mask[0, 0] and mask.sum() == mask.size - 1                # every collected pixel: the stamp is smaller than the 20 pixels
		probs = halo.build_problems(images, quality, mask, seg)
		fitted = [int(np.sum(p.fit)) for p in probs]
		assert all(len(p.pix) >= 1 for p in probs)
		assert (min(fitted) < 3) == (f == cc.DEGENERATE), (cc.FILES[f], fitted)
	assert tuple(switching) == cc.SWITCHING
	assert tuple(f for f in n_seg if n_seg[f] == 2) == cc.TWO_SEGMENTS and all(k in (1, 2) for k in n_seg.values())
	tmags = [float(s.target_tmag[i]) for s, i, _, _, _ in spec]
	assert sum(t <= tmag_limit for t in tmags) == 4 and tmags[4] > tmag_limit and tmags[5] > tmag_limit
