# -*- coding: utf-8 -*-
"""bench.py end to end on the GPU box, small: the stdout of a run is ONE short line the driver can parse (benchlib.line.check_line),
at N = 1 and -- two ranks sharing the one device: a control-flow run through the host group -- at N = 2, started both ways
(spawned by bench.py itself, and by torch.distributed.run as the driver does)."""
import json
import os
import subprocess
import sys
import pytest
from benchlib import line as bl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--steps', '3', '--warmup', '1', '--targets', '512', '--cadences', '200', '--cpu-sample', '0', '--no-extra']


def _run(cmd, tmp_path):
	env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'TESSPHOT_RDZV_ID')}
	r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
	assert r.returncode == 0, r.stderr.decode()[-3000:]
	out = r.stdout.decode().strip().splitlines()
	assert len(out) == 1, out                       # nothing but the line on stdout
	return bl.check_line(out[0])


def test_single_gpu_line(tmp_path):
	d = _run([sys.executable, 'bench.py', '--gpus', '1'] + SMALL, tmp_path)
	assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1 and d['value'] > 0
	assert d['config']['workload'].startswith('configs[2]') and d['roofline']['frac'] > 0
	full = json.load(open(os.path.join(ROOT, bl.LEGS_FILE)))
	assert full['value'] == pytest.approx(d['value'], rel=1e-5) and 'kernels' in full


def test_plain_run_measures_the_headline_only(tmp_path):
	"""Without --full nothing runs beside the warm-up and the timed steps: no CPU baseline and no extra leg in the full result."""
	d = _run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1', '--targets', '512', '--cadences', '200'], tmp_path)
	full = json.load(open(os.path.join(ROOT, bl.LEGS_FILE)))
	assert full['value'] == pytest.approx(d['value'], rel=1e-5) and 'legs' not in d
	for k in ('cpu_baseline', 'parity_sample', 'aperture_premade_cubes', 'stages', 'end_to_end', 'linpsf', 'frames_to_results',
			'psf_frames_to_results', 'psf_fit', 'fit_background_frames', 'frames_to_results_large_batch'):
		assert k not in full, k
	kernels = full['kernels']
	assert kernels['tp_bkg_stamp_sum_kernel']['launches'] == 2 and kernels['tp_aperture_fused_kernel']['launches'] == 2


def test_dump_outputs_of_the_last_step(tmp_path):
	"""--dump-outputs: the arrays of the last timed step in float32 / float64, every file finite (the NaN of the light curves in
	their _nonfinite files), under 64 MB, the same from run to run (seeded inputs); --steps sets the number of timed steps."""
	import numpy as np
	from benchlib import dump
	dumps = []
	for k, steps in enumerate(('2', '4')):
		d = str(tmp_path / str(k))
		line = _run([sys.executable, 'bench.py', '--gpus', '1', '--dump-outputs', d] + SMALL + ['--steps', steps], tmp_path)
		assert line['steps'] == int(steps) and line['ms_per_step'] > 0
		kernels = json.load(open(os.path.join(ROOT, bl.LEGS_FILE)))['kernels']    # launches in the timed region: one of each per step
		assert kernels['tp_bkg_stamp_sum_kernel']['launches'] == int(steps) and kernels['tp_aperture_fused_kernel']['launches'] == int(steps)
		dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)})
		assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= dump.MAX_BYTES
	a, b = dumps
	assert set(a) == {'lc', 'lc_nonfinite', 'contamination', 'contamination_nonfinite', 'status', 'flags', 'mask', 'target_index'}
	assert a['lc'].shape == a['lc_nonfinite'].shape == (5, 512, 200)
	for name in a:
		assert a[name].dtype in (np.float32, np.float64) and np.isfinite(a[name]).all(), name
		np.testing.assert_array_equal(a[name], b[name], err_msg=name)
	# the cubes carry NaN pixels: the flux of a cadence with one in the mask is NaN (the reference's np.sum), a code of 1 here
	assert (a['lc'][0] != 0).any() and (a['lc_nonfinite'][0] == 1).any() and (a['mask'] > 0).any()


@pytest.mark.parametrize('launcher', ['own', 'torchrun'])
def test_two_ranks_on_one_device_line(tmp_path, launcher):
	if launcher == 'own':
		cmd = [sys.executable, 'bench.py', '--gpus', '2'] + SMALL
	else:
		pytest.importorskip('torch')
		cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
			'--master-port', str(26500 + os.getpid() % 2000), 'bench.py', '--gpus', '2'] + SMALL
	d = _run(cmd, tmp_path)
	assert d['n_gpus'] == 2 and d['config']['workload'].startswith('configs[4]') and d['config']['targets_total'] == 1024
	g = d['gather']
	assert g['mode'].startswith('host') and g['issued_short'] in ('step', 'final') and g['measured_8gpu'] is False
	assert g['step_ms_without_gather'] > 0 and (g['mean_ms'] or g['final_ms'])
	assert 'warning' in d                           # two ranks on one GPU: said so in the line
