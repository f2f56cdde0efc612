#!/usr/bin/env python
"""HIP-event times of the camera-table kernels (nrf_camera_table_rays / _rays_backward) next to the by-value
nrf_camera_pixels_to_rays on a 960x540 frame, as markdown:
    python scripts/bench_camera_table.py >> profiles/camera_grads.md
Each figure: 20 warm-up calls, then the median over 200 events-bracketed calls on the current stream."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_sha)
from nerfies_amd import lib as L  # noqa: E402
from nerfies_amd.camera import Camera, pack_cameras  # noqa: E402

WARMUP, REPS = 20, 200


def median_us(fn):
  for _ in range(WARMUP):
    fn()
  torch.cuda.synchronize()
  ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
  for a, b in ev:
    a.record()
    fn()
    b.record()
  torch.cuda.synchronize()
  t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
  return t[len(t) // 2], t[len(t) // 10], t[-len(t) // 10]


def cameras(num, rng, size=(960, 540)):
  out = []
  for _ in range(num):
    R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    out.append(Camera(orientation=R, position=rng.normal(size=3), focal_length=800.0, principal_point=[size[0] / 2 + 0.2, size[1] / 2 - 0.3],
                      image_size=list(size), skew=0.3, pixel_aspect_ratio=1.02, radial_distortion=[0.05, -0.02, 0.004],
                      tangential_distortion=[0.001, -0.002]))
  return out


def main():
  lib = L.load_library()
  dev = torch.device('cuda:0')
  rng = np.random.default_rng(0)
  st = torch.cuda.current_stream().cuda_stream
  print(f'\n## Timings ({torch.cuda.get_device_name(0)}, csrc_sha16 {bench.kernel_source_sha()})\n')
  print(f'HIP events around each call, {WARMUP} warm-up calls, median of {REPS} (10th .. 90th percentile); distorted cameras.\n')
  print('| call | n | C | index | median us | p10 .. p90 us |')
  print('|---|---|---|---|---|---|')
  cam = cameras(1, rng)[0]
  n = 960 * 540
  o, d, p = (torch.empty((n, k), device=dev) for k in (3, 3, 2))
  desc = cam._desc()
  m = median_us(lambda: lib.nrf_camera_pixels_to_rays(desc, None, n, o.data_ptr(), d.data_ptr(), p.data_ptr(), st))
  print(f'| nrf_camera_pixels_to_rays (pixel centres generated, pixels written) | {n} | by value | - | {m[0]:.1f} | {m[1]:.1f} .. {m[2]:.1f} |')
  m = median_us(lambda: lib.nrf_camera_pixels_to_rays(desc, p.data_ptr(), n, o.data_ptr(), d.data_ptr(), None, st))
  print(f'| nrf_camera_pixels_to_rays (explicit pixels) | {n} | by value | - | {m[0]:.1f} | {m[1]:.1f} .. {m[2]:.1f} |')
  for n, num, random in ((518400, 1, False), (6144, 64, True), (49152, 512, True)):
    table = pack_cameras(cameras(num, rng), dev)
    idx = torch.from_numpy(rng.integers(0, num, n).astype(np.int32)).to(dev) if random else None
    ip = idx.data_ptr() if random else None
    px = torch.from_numpy(rng.uniform(0, [960, 540], size=(n, 2)).astype(np.float32)).to(dev)
    o, d, g_o, g_d = (torch.randn((n, 3), device=dev) for _ in range(4))
    d_cam, d_px = torch.empty((num, 24), device=dev), torch.empty((n, 2), device=dev)
    b = C.c_size_t(0)
    L.check(lib.nrf_camera_table_workspace_bytes(n, num, C.byref(b)), lib)
    ws = torch.empty(b.value, dtype=torch.uint8, device=dev)
    tag = 'random' if random else 'NULL'
    fwd = lambda: lib.nrf_camera_table_rays(table.data_ptr(), num, ip, px.data_ptr(), n, o.data_ptr(), d.data_ptr(), st)
    bwd = lambda: lib.nrf_camera_table_rays_backward(table.data_ptr(), num, ip, px.data_ptr(), n, g_o.data_ptr(), g_d.data_ptr(),
                                                     d_cam.data_ptr(), d_px.data_ptr(), ws.data_ptr(), b.value, st)
    L.check(fwd(), lib)
    L.check(bwd(), lib)
    for name, fn in (('nrf_camera_table_rays', fwd), ('nrf_camera_table_rays_backward (two launches)', bwd)):
      m = median_us(fn)
      print(f'| {name} | {n} | {num} | {tag} | {m[0]:.1f} | {m[1]:.1f} .. {m[2]:.1f} |')
  print(f'\nWorkspace of the reverse pass: {b.value / n:.1f} B per ray.')


if __name__ == '__main__':
  main()
