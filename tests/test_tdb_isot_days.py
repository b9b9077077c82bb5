# -*- coding: utf-8 -*-
"""
``fitsio.tdb_to_utc_isot`` takes the whole days out of its two-part argument at once: the string is the one the day-by-day walk gave,
for every input, and the leap-second table is read a handful of times.  The yardstick is that walk, restated here as it stood.  No GPU.
"""
import numpy as np
import pytest
from photometry_amd import fitsio


def old_tdb_to_utc_isot(jd1, jd2=0.0):
	"""The function as it stood before the days were taken out: one turn of a loop, and one scan of the leap-second table, per day."""
	big, small = (jd1, jd2) if abs(jd1) >= abs(jd2) else (jd2, jd1)
	day = np.floor(big + 0.5)
	frac = (big - (day - 0.5)) + small
	mjd_day = int(day - 0.5 - 2400000.5 + 0.5)
	g = np.deg2rad(357.53 + 0.98560028 * ((big - 2451545.0) + small))
	sec = frac * 86400.0 - (0.001657 * np.sin(g) + 0.000014 * np.sin(2 * g)) - 32.184
	sec_utc = sec - fitsio._tai_minus_utc(mjd_day)
	while sec_utc < 0:
		mjd_day -= 1
		sec_utc = sec + 86400.0 * 1 - fitsio._tai_minus_utc(mjd_day)
		sec += 86400.0
	while sec_utc >= 86400.0:
		mjd_day += 1
		sec -= 86400.0
		sec_utc = sec - fitsio._tai_minus_utc(mjd_day)
	ms = int(np.floor(sec_utc * 1000.0 + 0.5))
	if ms >= 86400000:
		ms -= 86400000
		mjd_day += 1
	jdn = mjd_day + 2400001
	a = jdn + 32044
	b = (4 * a + 3) // 146097
	c = a - 146097 * b // 4
	d = (4 * c + 3) // 1461
	e = c - 1461 * d // 4
	m = (5 * e + 2) // 153
	dd = e - (153 * m + 2) // 5 + 1
	mm = m + 3 - 12 * (m // 10)
	yy = 100 * b + d - 4800 + m // 10
	hh, rem = divmod(ms, 3600000)
	mi, rem = divmod(rem, 60000)
	ss, ms = divmod(rem, 1000)
	return f'{yy:04d}-{mm:02d}-{dd:02d}T{hh:02d}:{mi:02d}:{ss:02d}.{ms:03d}'


def _grid():
	"""``(jd1, jd2)`` pairs: the same instants with the days split both ways and in both orders."""
	pairs = []
	# seconds around midnight (UTC midnight lies 69.184 s before TDB midnight in the TESS era: both are covered)
	near = np.concatenate([np.arange(-70.0, 70.5, 7.0), [-69.1845, -69.1835, -69.184, -0.0005, 0.0005, 37.0, 32.184, 69.1840001]]) / 86400.0
	days = [2457203.5, 2457204.5, 2457205.5, 2457753.5, 2457754.5, 2457755.5, 2458000.5, 2458324.5, 2459000.5, 2451544.5]   # 2015-07-01, 2017-01-01, TESS era, J2000
	for day in days:
		for off in near:
			whole = np.floor(day)
			pairs.append((day + off, 0.0))                              # one number
			pairs.append((whole, (day - whole) + off))                  # a whole day and the rest
			pairs.append((2457000.0, (day - 2457000.0) + off))          # the days in the small part, as the light-curve files call it
		for off in (near[::10] if day in (days[1], days[4]) else ()):
			pairs.append((2400000.5, (day - 2400000.5) + off))          # MJD form: 57 000 days for the old walk, so a few instants only
	# TESS-era (t, 2457000) pairs: sector starts and ends, half-hour steps through a day, a thousand days of noon and midnight
	rng = np.random.default_rng(4)
	ts = np.concatenate([[1000.49, 1325.29, 1353.17, 1683.35, 2000.0, 2000.5, 3000.25, 0.0, 0.25, 1.0, 1.5, 2.0, 2.0 - 1e-9, 3.0 - 1e-12, 4999.999999],
		1700.0 + np.arange(0, 720, 15) / 720.0, 1000.0 + np.arange(0, 1500, 37) * 0.5, rng.uniform(0.0, 5000.0, 150)])
	for t in ts:
		pairs.append((float(t), 2457000))
		pairs.append((2457000, float(t)))
	# negative small parts: the walk towards earlier days is left as it was
	for t in (-0.25, -1.0, -1.5, -30.75, -400.0 + 0.0008):
		pairs.append((2458000.5, t))
		pairs.append((t, 2458000.5))
	return pairs


def test_the_string_is_the_old_one_on_the_whole_grid():
	pairs = _grid()
	assert len(pairs) > 1200
	bad = []
	for jd1, jd2 in pairs:
		for a, b in ((jd1, jd2), (jd2, jd1)):
			got, want = fitsio.tdb_to_utc_isot(a, b), old_tdb_to_utc_isot(a, b)
			if got != want:
				bad.append((a, b, got, want))
	assert not bad, bad[:5]


def test_known_instants():
	assert fitsio.tdb_to_utc_isot(2458000.49) == fitsio.tdb_to_utc_isot(1000.49, 2457000) == old_tdb_to_utc_isot(1000.49, 2457000)
	assert fitsio.tdb_to_utc_isot(2451545.0).startswith('2000-01-01T11:58:55.816')          # J2000.0 TDB


def test_the_leap_second_table_is_read_a_handful_of_times(monkeypatch):
	calls = []
	plain = fitsio._tai_minus_utc

	def counted(mjd):
		calls.append(mjd)
		return plain(mjd)
	monkeypatch.setattr(fitsio, '_tai_minus_utc', counted)
	text = fitsio.tdb_to_utc_isot(1000.49, 2457000)
	n_new = len(calls)
	del calls[:]
	assert old_tdb_to_utc_isot(1000.49, 2457000) == text
	n_old = len(calls)
	assert n_new <= 8 < 1000 < n_old, (n_new, n_old)
	for jd1, jd2 in ((1325.29, 2457000), (2457000, 4999.9), (2400000.5, 58000.25)):
		del calls[:]
		fitsio.tdb_to_utc_isot(jd1, jd2)
		assert len(calls) <= 8, (jd1, jd2, len(calls))
