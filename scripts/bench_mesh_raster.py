#!/usr/bin/env python
"""Mesh rasteriser on one GPU, as markdown (profiles/mesh_raster.md):
    python scripts/bench_mesh_raster.py [--res 128 256] [--size 960 540] [--json out.json]
The workload of profiles/mesh.md: the canonical volume of the configuration-A model shape on a RES^3 grid over [-0.8, 0.8]^3, meshed at
the MEDIAN of the grid, seen by a distorted camera at (0, 0, -2.6) that holds the whole box in a 960 x 540 image.  Timed, on that mesh:
    density grid      evaluation.density_grid: what the mesh starts from
    project           nrf_camera_table_project_depth of the V vertices
    draw              nrf_mesh_raster_draw (clear, faces, scan, large, resolve), with barycentrics
    interpolate       nrf_mesh_raster_interpolate of one (V, 3) attribute
    visibility        nrf_mesh_raster_visibility
HIP events around each variant on the current stream; every variant is warmed up, then the variants ALTERNATE in one process for
--rounds rounds; median (10th .. 90th percentile).  Two draws are compared bit for bit before anything is timed.  Next to them stands
the documented cost of rendering the same 960 x 540 frame from the field (README.md: 2019 ms in float32, 218 ms in bfloat16)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_sha)
from nerfies_amd import camera as camera_lib, evaluation, lib as L, models  # noqa: E402
from scripts.bench_field_query import CfgA, WARMUP, pct  # noqa: E402

FIELD_FRAME_MS = {'float32': 2019.0, 'bfloat16': 218.0}   # README.md, a 960 x 540 frame through eval.py's renderer


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--res', type=int, nargs='+', default=[128, 256])
  ap.add_argument('--size', type=int, nargs=2, default=[960, 540], metavar=('W', 'H'))
  ap.add_argument('--rounds', type=int, default=30, help='timed runs of every variant')
  ap.add_argument('--json', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  frames = list(range(8))
  model, fp = models.construct_nerf(0, CfgA, 0, frames, [0, 1], frames, 0.0206, 0.826, device=dev)
  lib = model.lib
  stream = torch.cuda.current_stream(dev).cuda_stream
  device = torch.cuda.get_device_name(0)
  W, H = args.size
  cam = camera_lib.Camera(orientation=np.eye(3), position=(0.0, 0.0, -2.6), focal_length=0.45 * H / (0.8 / 1.8), principal_point=(W / 2, H / 2),
                          image_size=(W, H), radial_distortion=(0.05, -0.01, 0.0), tangential_distortion=(0.001, -0.001))
  table = camera_lib.pack_cameras([cam], dev)
  rec = {'device': device, 'csrc_sha16': bench.kernel_source_sha(), 'rounds': args.rounds, 'image': [W, H], 'grids': {}}
  for res in args.res:
    lo, hi = (-0.8,) * 3, (0.8,) * 3
    n = res ** 3
    sigma = evaluation.density_grid(model, fp, lo, hi, res)
    thr = float(sigma.reshape(-1).sort().values[n // 2])
    step = [1.6 / res] * 3
    origin = [-0.8 + 0.5 * s for s in step]
    mesh = evaluation.extract_mesh_from_grid(sigma, origin, step, thr, lib=lib)
    vertices, faces = mesh['vertices'], mesh['faces']
    V, F = vertices.shape[0], faces.shape[0]
    nbytes = C.c_size_t(0)
    L.check(lib.nrf_mesh_raster_workspace_bytes(F, W, H, C.byref(nbytes)), lib)
    ws = torch.empty((nbytes.value + 3) // 4, dtype=torch.int32, device=dev)
    screen = torch.empty(V, 3, device=dev)
    face_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    depth, bary = torch.empty(H, W, device=dev), torch.empty(H, W, 3, device=dev)
    attribute, value = torch.randn(V, 3, device=dev), torch.empty(H, W, 3, device=dev)
    visible = torch.empty(V, dtype=torch.uint8, device=dev)

    def project():
      L.check(lib.nrf_camera_table_project_depth(table.data_ptr(), 1, None, vertices.data_ptr(), V, screen.data_ptr(), stream), lib)

    def draw():
      L.check(lib.nrf_mesh_raster_draw(screen.data_ptr(), V, faces.data_ptr(), F, W, H, 0.0, face_id.data_ptr(), depth.data_ptr(), bary.data_ptr(),
                                       ws.data_ptr(), ws.numel() * 4, stream), lib)

    def interpolate():
      L.check(lib.nrf_mesh_raster_interpolate(face_id.data_ptr(), bary.data_ptr(), H * W, faces.data_ptr(), F, attribute.data_ptr(), V, 3, None,
                                              value.data_ptr(), stream), lib)

    def visibility():
      L.check(lib.nrf_mesh_raster_visibility(face_id.data_ptr(), H * W, faces.data_ptr(), F, V, visible.data_ptr(), stream), lib)

    project()
    draw()
    first = (face_id.clone(), depth.clone(), bary.clone())
    status = ws[:4].tolist()
    draw()
    assert torch.equal(first[0], face_id) and torch.equal(first[1].view(torch.int32), depth.view(torch.int32))
    assert torch.equal(first[2].view(torch.int32), bary.view(torch.int32)) and ws[:4].tolist() == status
    visibility()
    seen = int(visible.sum())
    variants = {'density grid': lambda: evaluation.density_grid(model, fp, lo, hi, res), 'project': project, 'draw': draw,
                'interpolate': interpolate, 'visibility': visibility}
    for fn in variants.values():
      for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
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
    med = {k: pct(ts) for k, ts in times.items()}
    frame = med['project'][0] + med['draw'][0] + med['interpolate'][0]
    rec['grids'][str(res)] = {'points': n, 'threshold': thr, 'V': V, 'F': F, 'status': status, 'visible_vertices': seen,
                              'workspace_bytes': nbytes.value, 'ms': {k: list(v) for k, v in med.items()}, 'frame_ms': frame,
                              'share_of_density_grid': frame / med['density grid'][0]}
    print(f'\n## {res}^3 grid: V = {V}, F = {F} into {W} x {H} ({device}, csrc_sha16 {rec["csrc_sha16"]})\n')
    print(f'Drawn triangles {status[0]}, of them on the workgroup path {status[1]}; covered pixels {status[2]} of {W * H}; visible vertices '
          f'{seen}.  Workspace {nbytes.value} B.  Two draws gave the same bits.\n')
    print('| what | runs | ms (10th .. 90th percentile) |')
    print('|---|---|---|')
    for k, (m, l, h) in med.items():
      print(f'| {k} | {len(times[k])} | {m:.3f} ({l:.3f} .. {h:.3f}) |')
    print(f'| the same frame rendered from the field (README.md), float32 / bfloat16 | - | {FIELD_FRAME_MS["float32"]:.0f} / {FIELD_FRAME_MS["bfloat16"]:.0f} |')
    print(f'\n- project + draw + interpolate: {frame:.3f} ms, {100 * frame / med["density grid"][0]:.2f} % of the density grid of the same run, '
          f'1 / {FIELD_FRAME_MS["float32"] / frame:.0f} of the float32 field render of the frame.', flush=True)
  if args.json:
    with open(args.json, 'w') as f:
      json.dump(rec, f, indent=1)


if __name__ == '__main__':
  main()
