#!/usr/bin/env python
"""Cost of a deeper rgb branch: the config-A training step (1024 rays x (64 + 128) samples, F_p = 8, view directions, stratified
sampling, float32 mode, loss + gradients + Adam) at ModelConfig.nerf_rgb_branch_depth = 1, 2, 4 through the public Python API.
bench.py measures the one-layer model only and has no switch for the depth; this is the report next to it.

    python scripts/bench_rgb_depth.py [--depths 1 2 4] [--rays 1024] [--window-s 2.0]

Per depth: 10 warm-up steps, then whole steps until the window has passed, between two device synchronisations on the host clock;
prints one JSON line with rays/s per depth and the slow-down against depth 1.  From shapes an extra 128 x 128 layer is
3 x 2 x 128 x 128 = 98.3 kFLOP per sample over forward, dgrad and wgrad against 3.46 MFLOP of the step: + 2.8 % per extra layer."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerfies_amd import models, training  # noqa: E402


def rate(depth, rays, window_s, warmup):
  class Cfg:
    num_coarse_samples, num_fine_samples, num_nerf_point_freqs = 64, 128, 8
    sigma_activation, use_stratified_sampling, use_viewdirs = 'softplus', True, True
    nerf_rgb_branch_depth = depth
  dev = 'cuda:0'
  model, fp = models.construct_nerf(0, Cfg, rays, [0, 1, 2, 3], [0, 1], [0, 1, 2, 3], 0.05, 1.0, device=dev)
  state = training.TrainState(optimizer=training.Optimizer(fp))
  g = torch.Generator().manual_seed(1)
  batch = {'origins': (torch.rand(rays, 3, generator=g) - 0.5).to(dev),
           'directions': torch.nn.functional.normalize(torch.randn(rays, 3, generator=g), dim=-1).to(dev),
           'rgb': torch.rand(rays, 3, generator=g).to(dev), 'metadata': {}}
  sp = training.ScalarParams(learning_rate=1e-4)
  key = 0
  for _ in range(warmup):
    state, _, key = training.train_step(model, key, state, batch, sp)
  torch.cuda.synchronize()
  steps, t0 = 0, time.perf_counter()
  while True:
    for _ in range(10):
      state, stats, key = training.train_step(model, key, state, batch, sp)
    steps += 10
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dt >= window_s:
      break
  ws_bytes = model.workspace(rays, True, dev).numel() * 4
  return dict(depth=depth, rays_per_s=rays * steps / dt, steps=steps, window_s=dt, loss_rgb_fine=float(stats['fine']['loss/rgb']),
              train_workspace_bytes=ws_bytes)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--depths', type=int, nargs='+', default=[1, 2, 4])
  ap.add_argument('--rays', type=int, default=1024)
  ap.add_argument('--window-s', type=float, default=2.0)
  ap.add_argument('--warmup', type=int, default=10)
  a = ap.parse_args()
  rows = [rate(d, a.rays, a.window_s, a.warmup) for d in a.depths]
  base = next((r['rays_per_s'] for r in rows if r['depth'] == 1), None)
  for r in rows:
    r['slowdown_vs_depth1'] = (base / r['rays_per_s'] - 1.0) if base else None
  print(json.dumps({'bench': 'rgb_branch_depth', 'rays': a.rays, 'results': rows}))


if __name__ == '__main__':
  main()
