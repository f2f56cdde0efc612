#!/usr/bin/env python
"""Gradient-query throughput on one GPU, as markdown (profiles/field_gradient.md):
    python scripts/bench_field_gradient.py [--json out.json]
The workload of profiles/field_query.md: a 128^3 grid (2 097 152 points) at the configuration-A model shape (8 x 256 trunk, F_p = 8,
softplus), without and with an SE3 field (num_warp_freqs = 8), four ways:
    canonical / density-only     nrf_query_grid, one call                        (what the parent commit has)
    canonical / gradient         nrf_query_grid_grad, two calls of 2^20 points   (sigma, grad_sigma, normals)
    warp / density-only          the same through the warp field
    warp / gradient
Yardstick: what a user can do without the gradient entries -- central differences, SIX density-only queries per point.
HIP events around each variant's calls on the current stream; every variant is warmed up, then the variants ALTERNATE in one process
until each has at least --window-s seconds of timed calls; median (10th .. 90th percentile).  Per launch group: device time from
nrf_profile_read (events around the launch), FLOPs from the shapes (2 per MAC, dense layers, unpadded: density_flops_row /
density_bwd_flops_row in csrc/nrf_run.hip) against the 157.3 TF fp32-MFMA peak.  Run the command twice to see the spread."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_sha)
from nerfies_amd import lib as L, models  # noqa: E402
from scripts.bench_field_query import CfgA, CfgWarp, PEAK_TF, RES, N, WARMUP, pct  # noqa: E402

CHUNK = L.NRF_QUERY_GRAD_MAX_POINTS


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--window-s', type=float, default=1.0, help='timed seconds per variant at least')
  ap.add_argument('--json', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  frames = list(range(8))
  mA, pA = models.construct_nerf(0, CfgA, 0, frames, [0, 1], frames, 0.0206, 0.826, device=dev)
  mW, pW = models.construct_nerf(0, CfgWarp, 0, frames, [0, 1], frames, 0.0206, 0.826, device=dev)
  origin, step, dims = [-0.8 + 0.8 / RES] * 3, [1.6 / RES] * 3, (RES, RES, RES)
  wid = {'warp': torch.tensor([[3]], dtype=torch.int32, device=dev)}
  sig = lambda: {'sigma': torch.empty(N, device=dev)}
  grad = lambda: {'sigma': torch.empty(N, device=dev), 'grad_sigma': torch.empty(N, 3, device=dev), 'normals': torch.empty(N, 3, device=dev)}
  outs = {'dA': sig(), 'gA': grad(), 'dW': sig(), 'gW': grad()}

  def gradient(m, p, out, **kw):
    for first in range(0, N, CHUNK):
      count = min(CHUNK, N - first)
      m.query_grid_gradient(p, origin, step, dims, first, count, {k: v[first:first + count] for k, v in out.items()}, workspace_points=CHUNK, **kw)

  wkw = dict(metadata=wid, warp_extra={'alpha': 8.0})
  variants = {
      'canonical / density-only': lambda: mA.query_grid(pA, origin, step, dims, 0, N, outs['dA']),
      'canonical / gradient': lambda: gradient(mA, pA, outs['gA']),
      'warp (SE3, F_w = 8) / density-only': lambda: mW.query_grid(pW, origin, step, dims, 0, N, outs['dW'], **wkw),
      'warp (SE3, F_w = 8) / gradient': lambda: gradient(mW, pW, outs['gW'], **wkw),
  }
  for fn in variants.values():
    for _ in range(WARMUP):
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in variants}
  while min(sum(t) for t in times.values()) < args.window_s * 1e3:
    evs = []
    for k, fn in variants.items():   # alternate: one pass over the grid of each per round
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      evs.append((k, a, b))
    torch.cuda.synchronize()
    for k, a, b in evs:
      times[k].append(a.elapsed_time(b))
  assert bool(torch.equal(outs['dA']['sigma'], outs['gA']['sigma'])), 'canonical: the gradient query and the density-only query give different sigma'
  assert bool(torch.equal(outs['dW']['sigma'], outs['gW']['sigma'])), 'warp: the gradient query and the density-only query give different sigma'
  assert bool(torch.isfinite(outs['gW']['grad_sigma']).all() and torch.isfinite(outs['gA']['normals']).all())

  regions = {}
  for k, fn in variants.items():
    m = mW if k.startswith('warp') else mA
    m.profile_enable(True)
    for _ in range(10):
      fn()
    torch.cuda.synchronize()
    # per pass over the grid: a gradient pass is two calls, so a region's launches are summed over them
    regions[k] = {p['name']: (p['ms'] / 10.0, p['flops_per_launch'] * p['launches'] / 10.0) for p in m.profile_read()}
    m.profile_enable(False)

  device = torch.cuda.get_device_name(0)
  rec = {'device': device, 'csrc_sha16': bench.kernel_source_sha(), 'points': N, 'chunk': CHUNK, 'window_s': args.window_s, 'variants': {},
         'regions': regions}
  print(f'\n## 128^3 grid, {N} points per pass ({device}, csrc_sha16 {rec["csrc_sha16"]})\n')
  print(f'HIP events around each pass over the grid, {WARMUP} warm-up passes per variant, the variants alternating in one process until each '
        f'has {args.window_s:g} s of timed passes; median (10th .. 90th percentile).  A gradient pass is {-(-N // CHUNK)} calls of {CHUNK} points.\n')
  print('| variant | passes | ms per pass | points/s | in density-only queries of the same build | against six of them (central differences) |')
  print('|---|---|---|---|---|---|')
  med = {k: pct(ts) for k, ts in times.items()}
  for k, ts in times.items():
    m, lo, hi = med[k]
    base = med[k.split(' / ')[0] + ' / density-only'][0]
    rec['variants'][k] = {'passes': len(ts), 'ms': [m, lo, hi], 'points_per_s': N / (m * 1e-3), 'density_queries': m / base}
    print(f'| {k} | {len(ts)} | {m:.3f} ({lo:.3f} .. {hi:.3f}) | {N / (m * 1e-3):.4g} | {m / base:.2f} | {m / (6 * base):.2f} x |', flush=True)
  print('\nLaunch groups of one pass (nrf_profile_read: ms per pass, and TF/s where the group has a flop count):\n')
  for k, reg in regions.items():
    parts = []
    for n, (ms, flops) in reg.items():
      tf = flops / (ms * 1e-3) / 1e12 if flops > 0 and ms > 0 else 0.0
      parts.append(f'{n} {ms:.3f}' + (f' ({tf:.1f} TF/s, {100 * tf / PEAK_TF:.0f} %)' if tf else ''))
    print(f'- {k}: ' + ', '.join(parts))
  if args.json:
    with open(args.json, 'w') as f:
      json.dump(rec, f, indent=1)


if __name__ == '__main__':
  main()
