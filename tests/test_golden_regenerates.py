# -*- coding: utf-8 -*-
"""
The first link of the parity chain: the generators under tests/golden/ execute the reference and write the fixtures that
``oracle/`` is pinned to.  These tests run every generator again, into a temporary directory, and hold what it writes to the
committed files by content: for ``.npz`` the same keys and per key the same dtype, shape and raw bytes (NaN payloads and signed
zeros count), for ``.json`` the same parsed document.  No tolerance anywhere.

Every generator runs in a fresh interpreter: they install import hooks and mock modules.  After each run ``tests/golden`` must
be byte for byte what it was, and ``git status --porcelain tests/golden`` must be empty where the tree is a git checkout -- so
run these tests on a tree whose ``tests/golden`` is committed.

CPU only, and only where the reference checkout is present (skipped otherwise: it never travels to the GPU machine).
About 2 minutes in all: 9 s per full run of make_golden.py, 2 to 4 s per single fixture, 3 s for the motion fixture and 65 s for
the PSF-distribution sample.
"""
import glob
import hashlib
import json
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
from _refstub import REFERENCE_PATH # noqa: E402  (the probe of missing packages it runs on import changes nothing)

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE_PATH, 'photometry')),
	reason=f"the reference checkout ({REFERENCE_PATH}) is not on this machine: the fixtures cannot be regenerated here")

# make_golden.py's default list, in its order; ``test_default_order`` holds the generator to it
DEFAULT = ['misc', 'sumimage', 'aperture', 'k2p2', 'psf', 'linpsf', 'diagnostics', 'cutout', 'background', 'psfphot', 'pixelflags',
	'shenanigans', 'skiptargets', 'fitsfile']


def files_of(name):
	return ['golden_fitsfile.json', 'golden_fitsfile.npz'] if name == 'fitsfile' else [f'golden_{name}.npz']


# which test regenerates which fixture; a fixture on neither list fails test_every_fixture_is_accounted_for
REGENERATED = {f for name in DEFAULT for f in files_of(name)} | {'golden_motion.npz', 'golden_psf_distribution.npz'}
# golden_wcs.npz needs astropy 4.3 (wcslib), which is not installed where these tests run.
NOT_REGENERATED = {'golden_wcs.npz'}
# golden_psf_distribution.npz is 21 minutes of the oracle on 7 processes: only PSF_SAMPLE of its 120 target rows are fitted again.
PSF_SAMPLE = 2


#--------------------------------------------------------------------------------------------------
def snapshot():
	"""sha256 of every file under tests/golden (interpreter caches aside)."""
	snap = {}
	for d, dirs, files in os.walk(GOLDEN):
		dirs[:] = [x for x in dirs if x != '__pycache__']
		for f in files:
			if not f.endswith('.pyc'):
				p = os.path.join(d, f)
				with open(p, 'rb') as fh:
					snap[os.path.relpath(p, GOLDEN)] = hashlib.sha256(fh.read()).hexdigest()
	return snap


def git_status():
	"""``git status --porcelain tests/golden``, or None where the tree is not a git checkout."""
	try:
		inside = subprocess.run(['git', 'rev-parse', '--is-inside-work-tree'], cwd=ROOT, capture_output=True, text=True, timeout=30)
	except OSError:
		return None
	if inside.returncode != 0 or inside.stdout.strip() != 'true':
		return None
	return subprocess.run(['git', 'status', '--porcelain', 'tests/golden'], cwd=ROOT, capture_output=True, text=True, timeout=30, check=True).stdout


def generate(script, args, out, timeout):
	"""Run a generator in a fresh interpreter into ``out``; tests/golden must come out of it untouched."""
	before = snapshot()
	cmd = [sys.executable, os.path.join(GOLDEN, script)] + [str(a) for a in args]
	r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
	assert r.returncode == 0, f"{' '.join(cmd)} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
	assert snapshot() == before, f"{script} changed files under tests/golden although --out names {out}"
	status = git_status()
	assert status is None or status == '', f"git status --porcelain tests/golden after {script}:\n{status}"
	return sorted(os.listdir(out))


def npz_differences(new_path, committed_path):
	"""What differs between two .npz files by content: key set, and per key dtype, shape and raw bytes."""
	diffs = []
	with np.load(new_path, allow_pickle=False) as new, np.load(committed_path, allow_pickle=False) as old:
		if set(new.files) != set(old.files):
			diffs.append(f"keys only regenerated {sorted(set(new.files) - set(old.files))}, only committed {sorted(set(old.files) - set(new.files))}")
		for k in sorted(set(new.files) & set(old.files)):
			a, b = new[k], old[k]
			if a.dtype != b.dtype or a.shape != b.shape:
				diffs.append(f"{k}: regenerated {a.dtype}{a.shape}, committed {b.dtype}{b.shape}")
			elif a.tobytes() != b.tobytes():
				if a.dtype.kind in 'fiub' and a.size:
					ne = (a != b) & ~((a != a) & (b != b)) if a.dtype.kind == 'f' else (a != b)
					diffs.append(f"{k}: {int(np.count_nonzero(ne))} of {a.size} values differ (others differ in bits only)"
						f", first regenerated {np.ravel(a)[np.argmax(ne)]!r} committed {np.ravel(b)[np.argmax(ne)]!r}")
				else:
					diffs.append(f"{k}: regenerated {a!r}, committed {b!r}")
	return diffs


def json_differences(new, old, path=''):
	"""Where two parsed JSON documents differ."""
	if type(new) is not type(old):
		return [f"{path}: regenerated {new!r}, committed {old!r}"]
	if isinstance(new, dict):
		diffs = [f"{path}: keys only regenerated {sorted(set(new) - set(old))}, only committed {sorted(set(old) - set(new))}"] if set(new) != set(old) else []
		return diffs + [d for k in new if k in old for d in json_differences(new[k], old[k], f'{path}/{k}')]
	if isinstance(new, list):
		diffs = [f"{path}: regenerated {len(new)} items, committed {len(old)}"] if len(new) != len(old) else []
		return diffs + [d for i, (x, y) in enumerate(zip(new, old)) for d in json_differences(x, y, f'{path}/{i}')]
	same = new == old or (isinstance(new, float) and new != new and old != old)
	return [] if same else [f"{path}: regenerated {new!r}, committed {old!r}"]


def assert_equal_committed(out, files):
	problems = {}
	for f in files:
		new, old = os.path.join(out, f), os.path.join(GOLDEN, f)
		if f.endswith('.json'):
			with open(new) as a, open(old) as b:
				diffs = json_differences(json.load(a), json.load(b))
		else:
			diffs = npz_differences(new, old)
		if diffs:
			problems[f] = diffs
	assert not problems, "regenerated fixtures differ from the committed ones:\n" + '\n'.join(
		f"  {f}: {len(d)} difference(s)\n    " + '\n    '.join(d[:6]) + ('\n    ...' if len(d) > 6 else '') for f, d in problems.items())


#--------------------------------------------------------------------------------------------------
def test_default_order(tmp_path):
	"""``python tests/golden/make_golden.py``, the documented usage: every fixture it writes is the committed one, and it writes
	exactly the fixtures of DEFAULT.  (Before the k2p2FixFromSum patch of golden_aperture / golden_diagnostics was undone properly,
	this run recorded the patch's prescribed masks in golden_k2p2.npz, and golden_fitsfile.json carried the day of the run.)"""
	written = generate('make_golden.py', ['--out', tmp_path], tmp_path, timeout=180)
	expected = sorted(f for name in DEFAULT for f in files_of(name))
	assert written == expected
	assert_equal_committed(tmp_path, expected)


@pytest.mark.parametrize('name', DEFAULT)
def test_each_fixture_alone(tmp_path, name):
	"""``make_golden.py NAME`` alone writes the committed file(s) of NAME: no fixture depends on a generator that ran before it."""
	written = generate('make_golden.py', [name, '--out', tmp_path], tmp_path, timeout=90)
	assert written == sorted(files_of(name))
	assert_equal_committed(tmp_path, written)


def test_reversed_order(tmp_path):
	"""The default list backwards: no generator leaves state behind that changes one that runs after it."""
	written = generate('make_golden.py', ['--out', tmp_path] + DEFAULT[::-1], tmp_path, timeout=180)
	assert_equal_committed(tmp_path, written)
	assert written == sorted(f for name in DEFAULT for f in files_of(name))


def test_motion(tmp_path):
	written = generate('make_golden_motion.py', ['--out', tmp_path], tmp_path, timeout=90)
	assert written == ['golden_motion.npz']
	assert_equal_committed(tmp_path, written)


def psf_sample_targets(nit, nstars, n):
	"""The ``n`` targets with the smallest total iteration count, the last of them replaced by the cheapest target with more than
	one fitted star if there is none among them."""
	total = nit.astype('int64').sum(axis=1)
	order = [int(i) for i in np.argsort(total, kind='stable')]
	picked = order[:n]
	if not any(nstars[i] > 1 for i in picked):
		picked[-1] = next(i for i in order if nstars[i] > 1)
	return picked


def test_psf_distribution_sample(tmp_path):
	"""``make_psf_distribution.py --targets`` on the cheapest target of the committed ``nit`` and the cheapest one with more than
	one fitted star (targets 30 and 77: 1674 and 5128 simplex iterations over the 20 cadences, one and two stars): their rows
	equal the committed rows bit for bit.  Measured: 65 s wall on two processes, of which 64 s are target 77 (target 30 alone:
	14 s).  Every target with more than one star costs at least that, so the sample stays at two targets."""
	import make_psf_distribution as mk
	from oracle import psf_photometry as opp
	with np.load(os.path.join(GOLDEN, 'golden_psf_distribution.npz'), allow_pickle=False) as g:
		committed = {k: g[k] for k in g.files}
	s, _prf = mk.build_scene()
	nstars = [len(opp.select_stars(s.catalog_of(i), s.target_pos_row[i] - s.stamps[i][0], s.target_pos_column[i] - s.stamps[i][2],
		s.target_tmag[i])) for i in range(mk.NT)]
	targets = psf_sample_targets(committed['nit'], nstars, PSF_SAMPLE)
	assert len(set(targets)) == PSF_SAMPLE and any(nstars[i] > 1 for i in targets)
	written = generate('make_psf_distribution.py', ['--out', tmp_path, '--targets', ','.join(str(i) for i in targets)], tmp_path, timeout=600)
	assert written == ['golden_psf_distribution.npz']
	with np.load(os.path.join(tmp_path, written[0]), allow_pickle=False) as g:
		new = {k: g[k] for k in g.files}
	assert set(new) == set(committed) | {'targets'}
	assert new['targets'].tolist() == targets
	for k in committed:
		want = committed[k][targets] if k in ('flux', 'nit', 'pos_centroid', 'status') else committed[k]
		assert new[k].dtype == want.dtype and new[k].shape == want.shape, k
		assert new[k].tobytes() == np.ascontiguousarray(want).tobytes(), f"{k} of targets {targets}: regenerated {new[k]!r}, committed {want!r}"


def test_every_fixture_is_accounted_for():
	"""A fixture is either regenerated by a test of this file or listed, with its reason, as not regenerated here: the only one
	that is not is golden_wcs.npz (and the rows of golden_psf_distribution.npz outside the sample)."""
	assert NOT_REGENERATED == {'golden_wcs.npz'}
	assert not (REGENERATED & NOT_REGENERATED)
	present = {os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, 'golden_*'))}
	assert REGENERATED | NOT_REGENERATED == present
	with np.load(os.path.join(GOLDEN, 'golden_psf_distribution.npz'), allow_pickle=False) as g:
		assert 0 < PSF_SAMPLE < g['nit'].shape[0]
