"""bench.py's plain line (no --full): only what the headline figure needs runs -- no per-kernel profile, roofline, CPU baseline or
certificates -- `--steps` sets the timed steps, and --dump-outputs writes what the last timed step returned, from inputs that are
the same in every run (the time-based burn-in does not change them).  Runs bench.py in child processes, as the driver does."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
  env = dict(os.environ)
  for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'BENCH_FORCE_DIST', 'BENCH_DIST_BACKEND', 'BENCH_SAME_DEVICE', 'BENCH_BF16'):
    env.pop(k, None)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, capture_output=True, text=True, timeout=600,
                     cwd=ROOT)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, lines
  return json.loads(lines[0])


def _close(x, y, rel):
  """Equal up to the order of float sums: max |x - y| within `rel` of the array's largest magnitude."""
  x, y = x.astype(np.float64), y.astype(np.float64)
  return float(np.abs(x - y).max()) <= rel * max(float(np.abs(x).max()), 1e-30)


def test_plain_line_and_dumped_outputs(tmp_path):
  a, b = tmp_path / 'a', tmp_path / 'b'
  da = _bench(['--gpus', '1', '--steps', '20', '--warmup', '3', '--burn-in-s', '0.5', '--dump-outputs', str(a)])
  db = _bench(['--gpus', '1', '--steps', '20', '--warmup', '3', '--burn-in-s', '0', '--dump-outputs', str(b)])
  for d in (da, db):
    assert d['steps'] == 20 and d['warmup'] == 3 and d['unit'] == 'rays/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert d['metric'] == 'train rays/sec (192 samples/ray)' and d['n_gpus'] == 1
    assert d['ms_per_step'] > 0 and abs(d['value'] - 1024 * 1e3 / d['ms_per_step']) <= 1e-6 * d['value']
    assert d['full'] is False
    assert not {'roofline', 'kernels', 'cpu_baseline', 'eval_parity', 'secondary', 'sustained'} & set(d), sorted(d)
  assert da['steady_state']['burn_in_steps'] > 0 and db['steady_state']['burn_in_steps'] == 0
  names = sorted(os.listdir(a))
  assert names == sorted(os.listdir(b))
  assert {'params.npy', 'adam_m.npy', 'adam_v.npy', 'grad.npy', 'stats.fine.loss_rgb.npy', 'stats.coarse.loss_rgb.npy'} <= set(names)
  assert sorted(n + '.npy' for n in da['dumped_outputs']) == [n for n in names if not n.endswith('.index.npy')]
  assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
  for n in names:
    x, y = np.load(a / n), np.load(b / n)
    assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.isfinite(x).all(), n
  # the same 23 steps from the same parameters, batch and keys in both runs, with and without burn-in: the parameters stay the
  # seeded ones bit for bit, everything else agrees up to the order of the float atomics
  assert np.array_equal(np.load(a / 'params.npy'), np.load(b / 'params.npy'))
  for n in names:
    assert _close(np.load(a / n), np.load(b / n), 1e-5), n


def test_plain_eval_line_dumps_the_rendered_chunk(tmp_path):
  a, b = tmp_path / 'a', tmp_path / 'b'
  da = _bench(['--mode', 'eval', '--steps', '3', '--warmup', '1', '--burn-in-s', '0.3', '--dump-outputs', str(a)])
  _bench(['--mode', 'eval', '--steps', '3', '--warmup', '1', '--burn-in-s', '0', '--dump-outputs', str(b)])
  assert da['steps'] == 3 and da['ms_per_step'] > 0 and da['full'] is False and 'roofline' not in da and 'kernels' not in da
  for lv in ('coarse', 'fine'):
    rgb = np.load(a / f'{lv}.rgb.npy')
    assert rgb.shape == (8192, 3) and rgb.dtype == np.float32 and np.isfinite(rgb).all() and (rgb >= 0).all() and (rgb <= 1).all()
  assert sorted(os.listdir(a)) == sorted(os.listdir(b))
  for n in os.listdir(a):
    assert _close(np.load(a / n), np.load(b / n), 1e-6), n
