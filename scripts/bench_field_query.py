#!/usr/bin/env python
"""Field-query throughput on one GPU, as markdown (profiles/field_query.md):
    python scripts/bench_field_query.py [--json out.json]
A 128^3 grid (2 097 152 points, one nrf_query_grid call) at the configuration-A model shape (8 x 256 trunk, F_p = 8, view directions
with F_v = 4, softplus), three ways:
    canonical / density-only   (out->rgb == NULL: nerf_density_kernel)
    canonical / full           (sigma + rgb: the float32 forward chain + field_unpack)
    warp / full                (the same model with an SE3 field, num_warp_freqs = 8, queried through the warp)
HIP events around each call on the current stream; every variant is warmed up, then the variants ALTERNATE in one process until each has
at least --window-s seconds of timed calls; median (10th .. 90th percentile) and points/s.  The MLP kernel of each variant: device time
from nrf_profile_read (events around the launch), FLOPs from the shapes (2 per MAC, dense layers, unpadded), against the 157.3 TF
fp32-MFMA peak.  Yardstick for the full query: the inference `apply` forward on the same number of rows -- 4096 rays x (256 + 256)
samples, whose FINE level is 4096 x 512 = 2 097 152 rows through the same chain kernel, plus sampling and compositing -- from the same
process; its `mlp_fwd_fine` region is the chain kernel alone.  Run the command twice to see the spread."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_sha)
from nerfies_amd import models  # noqa: E402

PEAK_TF = 157.3   # fp32 MFMA, MI355X
RES = 128
N = RES ** 3
WARMUP = 5


class CfgA:   # configuration A's model; 256 + 256 samples so that the yardstick's fine level has N rows at 4096 rays
  num_coarse_samples, num_fine_samples = 256, 256
  num_nerf_point_freqs, num_nerf_viewdir_freqs = 8, 4
  sigma_activation = 'softplus'
  use_stratified_sampling = False
  use_viewdirs = True


class CfgWarp(CfgA):
  use_warp, num_warp_freqs, num_warp_features, warp_field_type = True, 8, 8, 'se3'


def pct(ts):
  ts = sorted(ts)
  return ts[len(ts) // 2], ts[len(ts) // 10], ts[-max(len(ts) // 10, 1)]


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
  view = torch.tensor([[0.0, 0.0, 1.0]], device=dev)
  wid = {'warp': torch.tensor([[3]], dtype=torch.int32, device=dev)}
  sig = lambda: {'sigma': torch.empty(N, device=dev)}
  full = lambda: {'sigma': torch.empty(N, device=dev), 'rgb': torch.empty(N, 3, device=dev)}
  outs = {'density': sig(), 'full': full(), 'warp': full()}
  variants = {
      'canonical / density-only': lambda: mA.query_grid(pA, origin, step, dims, 0, N, outs['density']),
      'canonical / full': lambda: mA.query_grid(pA, origin, step, dims, 0, N, outs['full'], viewdirs=view),
      'warp (SE3, F_w = 8) / full': lambda: mW.query_grid(pW, origin, step, dims, 0, N, outs['warp'], viewdirs=view, metadata=wid,
                                                          warp_extra={'alpha': 8.0}),
  }
  B = N // 512
  g = torch.Generator().manual_seed(0)
  d = torch.randn(B, 3, generator=g)
  rays = {'origins': (torch.rand(B, 3, generator=g) - 0.5).to(dev), 'directions': (d / d.norm(dim=-1, keepdim=True)).to(dev), 'metadata': {}}
  box = {}

  def yard():
    box['out'] = mA.apply(pA, rays, out=box.get('out'))
  variants['apply forward, 4096 rays x (256 + 256) (yardstick)'] = yard

  for fn in variants.values():
    for _ in range(WARMUP):
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in variants}
  while min(sum(t) for t in times.values()) < args.window_s * 1e3:
    evs = []
    for k, fn in variants.items():   # alternate: one call of each per round
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      evs.append((k, a, b))
    torch.cuda.synchronize()
    for k, a, b in evs:
      times[k].append(a.elapsed_time(b))
  assert bool(torch.equal(outs['density']['sigma'], outs['full']['sigma'])), 'density-only and full sigma differ'

  # per-region device times (events around each launch group), 10 calls each
  regions = {}
  for k, fn in variants.items():
    m = mW if k.startswith('warp') else mA
    m.profile_enable(True)
    for _ in range(10):
      fn()
    torch.cuda.synchronize()
    regions[k] = {p['name']: (p['ms'] / max(p['launches'], 1), p['flops_per_launch']) for p in m.profile_read()}
    m.profile_enable(False)

  device = torch.cuda.get_device_name(0)
  rec = {'device': device, 'csrc_sha16': bench.kernel_source_sha(), 'points': N, 'window_s': args.window_s, 'variants': {}, 'regions': regions}
  print(f'\n## 128^3 grid, {N} points per call ({device}, csrc_sha16 {rec["csrc_sha16"]})\n')
  print(f'HIP events around each call, {WARMUP} warm-up calls per variant, the variants alternating in one process until each has '
        f'{args.window_s:g} s of timed calls; median (10th .. 90th percentile).\n')
  print('| variant | calls | ms per call | points/s | MLP kernel ms | MLP kernel TF/s | of 157.3 TF | ns per row (MLP kernel) |')
  print('|---|---|---|---|---|---|---|---|')
  for k, ts in times.items():
    med, lo, hi = pct(ts)
    reg = regions[k]
    name = 'query_density' if 'query_density' in reg else 'query_mlp' if 'query_mlp' in reg else 'mlp_fwd_fine'
    ms, flops = reg[name]
    tf = flops / (ms * 1e-3) / 1e12
    rec['variants'][k] = {'calls': len(ts), 'ms': [med, lo, hi], 'points_per_s': N / (med * 1e-3), 'mlp_region': name, 'mlp_ms': ms,
                          'mlp_tf': tf, 'mlp_ns_per_row': ms * 1e6 / N}
    print(f'| {k} | {len(ts)} | {med:.3f} ({lo:.3f} .. {hi:.3f}) | {N / (med * 1e-3):.4g} | {ms:.3f} ({name}) | {tf:.1f} | {100 * tf / PEAK_TF:.1f} % | '
          f'{ms * 1e6 / N:.3f} |', flush=True)
  print('\nRegions of one call (nrf_profile_read, ms per launch group):\n')
  for k, reg in regions.items():
    print(f'- {k}: ' + ', '.join(f'{n} {ms:.3f}' for n, (ms, _) in reg.items()))
  if args.json:
    with open(args.json, 'w') as f:
      json.dump(rec, f, indent=1)


if __name__ == '__main__':
  main()
