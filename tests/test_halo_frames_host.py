# -*- coding: utf-8 -*-
"""
The batched Halo path without a GPU: the column predicate of the method switch against ``halo_switch_reason``, and the test region
of tests/test_gpu_halo_frames.py held to its conditions on the oracle alone.  (The counting rule the select kernel uses for
``nanmedian < minflux``, ``drop_pixel`` of csrc/halo_rules.h, is held to numpy in tests/test_halo_rules_host.py, which runs the C++.)
"""
import configparser
import numpy as np
import pytest
import halo_common as hc
import halo_frames_common as fc


# -- the switch predicate ------------------------------------------------------------------------------------------------------
class _Record(object):
	def __init__(self, tmag, status, errors=(), edge_flux=None, datasource='ffi'):
		self.target = {'tmag': tmag}
		self.status, self.datasource = status, datasource
		self._details = {'errors': list(errors)} if errors else {}
		if edge_flux is not None:
			self._details['edge_flux'] = edge_flux


def test_column_predicate_agrees_with_halo_switch_reason():
	import importlib
	tp = importlib.import_module('photometry_amd.tessphot')
	from photometry_amd.status import STATUS
	from photometry_amd.plugins import load_settings, mag2flux
	settings = load_settings()
	tmag_limit, flux_limit = settings.getfloat('haloswitch', 'tmag_limit'), settings.getfloat('haloswitch', 'flux_limit')
	expected = float(mag2flux(5.0))
	records = [
		(_Record(8.0, STATUS.ERROR, ['Too many stamp resizes.'], 10 * expected), None),                          # too faint
		(_Record(5.0, STATUS.ERROR, ['Too many stamp resizes.'], datasource='tpf:123'), None),                    # tpf datasource
		(_Record(5.0, STATUS.ERROR, ['Too many stamp resizes.']), tp._SWITCH_TEXT[1]),
		(_Record(5.0, STATUS.ERROR, ['Stamp resize hit limit. Haloswitch quick break.']), tp._SWITCH_TEXT[1]),
		(_Record(5.0, STATUS.OK, ['Too many stamp resizes.']), None),                                             # the message without the ERROR
		(_Record(5.0, STATUS.ERROR, ['something else']), None),
		(_Record(5.0, STATUS.OK, (), 2 * flux_limit * expected), tp._SWITCH_TEXT[2]),                             # edge flux above the limit
		(_Record(5.0, STATUS.OK, (), 0.5 * flux_limit * expected), None),                                         # and below
		(_Record(5.0, STATUS.ERROR, ['ERROR: Stamp resize hit limit. Haloswitch quick break.'], 2 * flux_limit * expected), tp._SWITCH_TEXT[2]),
		(_Record(tmag_limit, STATUS.OK, (), 10 * expected), tp._SWITCH_TEXT[2]),                                  # exactly at the magnitude limit
		(tp.FailedTask(['Traceback']), None),                                                                     # a failed task
	]
	for rec, want in records:
		assert tp.halo_switch_reason(rec, settings) == want, (rec.__dict__, want)
	# the same records as columns
	real = [r for r, _ in records]
	failed = np.array([isinstance(r, tp.FailedTask) for r in real])
	col = lambda f, fill: np.array([fill if isinstance(r, tp.FailedTask) else f(r) for r in real])
	codes = tp.halo_switch_codes(col(lambda r: r.target['tmag'], 0.0), col(lambda r: r.datasource.startswith('tpf:'), False), failed,
		col(lambda r: r.status == STATUS.ERROR, True), col(lambda r: any(m in r._details.get('errors', []) for m in tp._RESIZE_GAVE_UP), True),
		col(lambda r: r._details.get('edge_flux', np.nan), 1e30), tmag_limit, flux_limit)
	assert [tp._SWITCH_TEXT.get(int(c)) for c in codes] == [w for _, w in records]


# -- the region of the GPU tests, on the oracle alone --------------------------------------------------------------------------------
def test_region_meets_its_conditions_on_the_oracle():
	from oracle import aperture as oap, sumimage as osum
	frames, row0, col0, time, quality, cat, targets = fc.region()
	R, C, T = frames['images'].shape
	limits = (row0, row0 + R, col0, col0 + C)
	tmag_limit, flux_limit = 6.0, 0.01
	switched, kept = [], []
	for i, sid in enumerate(targets['starid']):
		tmag = float(targets['tmag'][i])
		o = oap.photometry_on_frames(oap.FrameTarget(frames, row0, col0, quality, cat, int(sid), tmag, float(targets['row'][i]), float(targets['column'][i])),
			haloswitch=(tmag_limit, flux_limit))
		if tmag > tmag_limit:
			continue
		edge_flux = o['details'].get('edge_flux')
		if edge_flux is not None and edge_flux / hc.mag2flux(tmag) > flux_limit:
			switched.append(int(sid))
		else:
			assert o['status'] in (1, 3) and 'mask' in o, (sid, o['status'], o['errors'])
			kept.append(int(sid))
	assert tuple(switched) == fc.BRIGHT_SWITCHING and len(switched) >= 3
	assert kept == [fc.BRIGHT_KEPT]
	seg = hc.segments(time, hc.split_times(2, time, np.zeros(T)))
	assert hc.split_times(2, time, np.zeros(T)) == (1368.0,) and seg.max() == 1
	assert np.any(quality & hc.DEFAULT_BITMASK)
	dropped_pixel = dropped_cadence = clipped = neighbour = 0
	for sid in switched:
		i = int(np.flatnonzero(targets['starid'] == sid)[0])
		st = fc.halo_stamp(limits, targets['row'][i], targets['column'][i])
		clipped += (st[1] - st[0]) * (st[3] - st[2]) < 23 * 23
		cube = frames['images'][st[0] - row0:st[1] - row0, st[2] - col0:st[3] - col0]
		mask = hc.pixel_mask(np.isfinite(osum.sumimage(cube, quality)).astype('int32'), st, targets['row'][i], targets['column'][i])
		probs = hc.problems(cube, quality, mask, seg)
		assert len(probs) == 2
		for k, p in enumerate(probs):
			dropped_pixel += len(p['pix']) < mask.sum()
			dropped_cadence += len(p['cad']) < np.count_nonzero(seg == k)
			assert p['fit'].sum() >= 3 and len(p['pix']) >= 1
		for sid2, r, c in zip(cat['starid'], cat['row'], cat['column']):
			rr, cc = int(np.round(r)) - st[0], int(np.round(c)) - st[2]
			if sid2 != sid and 0 <= rr < mask.shape[0] and 0 <= cc < mask.shape[1] and mask[rr, cc]:
				neighbour += 1
	assert dropped_pixel and dropped_cadence and clipped and neighbour
