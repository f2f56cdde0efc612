#!/usr/bin/env python
"""Inverse-warp throughput on one GPU, as markdown (profiles/unwarp.md):
    python scripts/bench_unwarp.py [--json out.json]
2^20 points in the scene's box at the configuration-A warp shape (SE3 field, 6 x 128 trunk, num_warp_freqs = 8), one id per point:
    warp                 nrf_warp_points, one call: the forward field on the same points   (what the parent commit has)
    unwarp, steps = K    nrf_unwarp_points, K in {1, 4, 8}, tolerance 0 (every row rides through every round)
The launch structure predicts, per round, one primal pass with its stash plus three tangent tiles per primal tile -- about four
forward passes -- plus the step kernel, and one closing primal pass per call.  The launch sequence does not depend on the data, so
neither does the time: the points and the (freshly initialised) field only have to be finite.
HIP events around each variant's call on the current stream; every variant is warmed up, then the variants ALTERNATE in one process
until each has at least --window-s seconds of timed calls; median (10th .. 90th percentile).  Per launch group: device time from
nrf_profile_read, FLOPs from the shapes (2 per MAC, dense layers, unpadded) against the 157.3 TF fp32-MFMA peak."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_sha)
from nerfies_amd import lib as L, models  # noqa: E402
from scripts.bench_field_query import CfgWarp, PEAK_TF, WARMUP, pct  # noqa: E402

N = L.NRF_UNWARP_MAX_POINTS
STEPS = (1, 4, 8)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--window-s', type=float, default=1.0, help='timed seconds per variant at least')
  ap.add_argument('--json', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  frames = list(range(8))
  model, params = models.construct_nerf(0, CfgWarp, 0, frames, [0, 1], frames, 0.0206, 0.826, device=dev)
  g = torch.Generator(device=dev).manual_seed(0)
  y = (torch.rand(N, 3, generator=g, device=dev) * 2 - 1) * 0.8
  ids = torch.randint(0, len(frames), (N,), generator=g, device=dev, dtype=torch.int32)
  we = {'alpha': 8.0}
  last = {}

  def unwarp(k):
    last[k] = model.unwarp_points(params, y, ids, we, steps=k, tolerance=0.0, max_step=0.25)

  variants = {'warp': lambda: model.warp_points(params, y, ids, we)}
  for k in STEPS:
    variants[f'unwarp, steps = {k}'] = lambda k=k: unwarp(k)
  for fn in variants.values():
    for _ in range(WARMUP):
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in variants}
  while min(sum(t) for t in times.values()) < args.window_s * 1e3:
    evs = []
    for k, fn in variants.items():
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      evs.append((k, a, b))
    torch.cuda.synchronize()
    for k, a, b in evs:
      times[k].append(a.elapsed_time(b))
  for k in STEPS:
    assert bool(torch.isfinite(last[k]['points']).all()), f'steps = {k}: a non-finite point'
  status = {k: [int((last[k]['status'] == s).sum()) for s in (0, 1, 2)] for k in STEPS}

  regions = {}
  model.profile_enable(True)
  for k in STEPS:
    name = f'unwarp, steps = {k}'
    model.profile_read()
    for _ in range(10):
      variants[name]()
    torch.cuda.synchronize()
    regions[name] = {p['name']: (p['ms'] / 10.0, p['flops_per_launch'] * p['launches'] / 10.0, p['launches'] // 10) for p in model.profile_read()}
  model.profile_enable(False)

  device = torch.cuda.get_device_name(0)
  rec = {'device': device, 'csrc_sha16': bench.kernel_source_sha(), 'points': N, 'window_s': args.window_s, 'variants': {}, 'regions': regions,
         'status': status}
  print(f'\n## {N} points per call ({device}, csrc_sha16 {rec["csrc_sha16"]})\n')
  print(f'HIP events around each call, {WARMUP} warm-up calls per variant, the variants alternating in one process until each has '
        f'{args.window_s:g} s of timed calls; median (10th .. 90th percentile).\n')
  print('| variant | calls | ms per call | points/s | in forward warps of the same build | forward warps per round |')
  print('|---|---|---|---|---|---|')
  med = {k: pct(ts) for k, ts in times.items()}
  base = med['warp'][0]
  prev = None
  for k, ts in times.items():
    m, lo, hi = med[k]
    steps = int(k.split('=')[1]) if '=' in k else 0
    # the slope between two step counts: the cost of one round without the call's fixed part (pack, closing pass)
    per_round = '' if not steps or prev is None else f'{(m - prev[1]) / (steps - prev[0]) / base:.2f}'
    rec['variants'][k] = {'calls': len(ts), 'ms': [m, lo, hi], 'points_per_s': N / (m * 1e-3), 'forward_warps': m / base}
    print(f'| {k} | {len(ts)} | {m:.3f} ({lo:.3f} .. {hi:.3f}) | {N / (m * 1e-3):.4g} | {m / base:.2f} | {per_round} |', flush=True)
    if steps:
      prev = (steps, m)
  print('\nLaunch groups of one call (nrf_profile_read: launches, ms per call, and TF/s where the group has a flop count):\n')
  for k, reg in regions.items():
    parts = []
    for n, (ms, flops, launches) in reg.items():
      tf = flops / (ms * 1e-3) / 1e12 if flops > 0 and ms > 0 else 0.0
      parts.append(f'{n} x{launches} {ms:.3f}' + (f' ({tf:.1f} TF/s, {100 * tf / PEAK_TF:.0f} %)' if tf else ''))
    print(f'- {k}: ' + ', '.join(parts))
  print('\nStatus of the rows after the call (0 out of steps / 1 converged / 2 stopped), on this freshly initialised field: '
        + '; '.join(f'steps = {k}: {v}' for k, v in status.items()))
  if args.json:
    with open(args.json, 'w') as f:
      json.dump(rec, f, indent=1)


if __name__ == '__main__':
  main()
