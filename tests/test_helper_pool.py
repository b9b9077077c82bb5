# -*- coding: utf-8 -*-
"""
CPU check of the frames engine's fork-join (HelperPool::fork_join, photometry_amd/csrc/helper_pool.h): the header compiled for the
host with ThreadSanitizer into the driver tests/hostsim/helper_pool_tsan.cpp.  Every part runs exactly once, exceptions reach the
caller, and TSan reports nothing (a helper that touched the caller's frame or the join state after the call returned would be a race).
"""
import os
import subprocess
import pytest
import conftest

SRC = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'helper_pool_tsan.cpp')
OUT_DIR = os.path.join(conftest.ROOT, 'tests', 'hostsim', 'build')
OUT = os.path.join(OUT_DIR, 'helper_pool_tsan')


@pytest.fixture(scope='module')
def driver():
	os.makedirs(OUT_DIR, exist_ok=True)
	subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=thread', '-Wall', '-pthread',
		'-I' + os.path.join(conftest.ROOT, 'photometry_amd', 'csrc'), '-o', OUT, SRC], check=True)
	return OUT


@pytest.mark.parametrize("case,expect", [('repeat', 'ok repeat 8000 fork-joins'), ('own_throws', 'ok own_throws own part'),
	('helper_throws', 'ok helper_throws')])
def test_fork_join_under_tsan(driver, case, expect):
	env = dict(os.environ, TSAN_OPTIONS='halt_on_error=1 exitcode=66')
	r = subprocess.run([driver, case], capture_output=True, text=True, timeout=600, env=env)
	assert 'ThreadSanitizer' not in r.stderr, r.stderr
	assert r.returncode == 0, (r.stdout, r.stderr)
	assert r.stdout.strip() == expect, r.stdout
