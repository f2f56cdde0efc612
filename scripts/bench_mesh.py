#!/usr/bin/env python
"""Mesh extraction on one GPU, as markdown (profiles/mesh.md):
    python scripts/bench_mesh.py [--res 128 256] [--json out.json]
The workload of profiles/field_query.md: the canonical volume of the configuration-A model shape (8 x 256 trunk, F_p = 8, softplus)
on a RES^3 grid over the same box, meshed at the MEDIAN of the grid (stated per grid), so that there is a real surface.  Timed:
    density grid            evaluation.density_grid (nrf_query_grid in chunks of 2^21 points): what the mesh starts from
    count                   nrf_mesh_count (classify + scan)
    emit                    nrf_mesh_emit (vertices + map, faces) into buffers of the counted sizes
    count + emit            both, back to back on the stream (the read-back of the two counts is not in it)
    device copy of the grid a plain tensor copy of the RES^3 floats: the HBM rate this box reaches on the same bytes
    inside bytes            (sigma > threshold) as one byte per sample, an elementwise pass that reads every sample ONCE: count's own
                            traffic without a single neighbour re-read, i.e. the floor of any LDS-staged classify
    density at V points     NerfModel.query_points(outputs=('sigma',)) at the mesh's vertices
    refine step             NerfModel.query_gradient(sigma, grad_sigma) at the vertices + nrf_mesh_snap
HIP events around each variant on the current stream; every variant is warmed up, then the variants ALTERNATE in one process for
--rounds rounds (a round runs each variant once: the variants differ by three orders of magnitude, so a time window per variant
would have the slow ones run for minutes); median (10th .. 90th percentile)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_sha)
from nerfies_amd import evaluation, lib as L, models  # noqa: E402
from scripts.bench_field_query import CfgA, WARMUP, pct  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--res', type=int, nargs='+', default=[128, 256])
  ap.add_argument('--rounds', type=int, default=40, help='timed runs of every variant')
  ap.add_argument('--json', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  frames = list(range(8))
  model, fp = models.construct_nerf(0, CfgA, 0, frames, [0, 1], frames, 0.0206, 0.826, device=dev)
  lib = model.lib
  stream = torch.cuda.current_stream(dev).cuda_stream
  device = torch.cuda.get_device_name(0)
  rec = {'device': device, 'csrc_sha16': bench.kernel_source_sha(), 'rounds': args.rounds, 'grids': {}}
  for res in args.res:
    lo, hi = (-0.8,) * 3, (0.8,) * 3
    n = res ** 3
    sigma = evaluation.density_grid(model, fp, lo, hi, res)
    flat = sigma.permute(2, 1, 0).reshape(-1)
    thr = float(flat.sort().values[n // 2])
    step = [1.6 / res] * 3
    origin = [-0.8 + 0.5 * s for s in step]
    grid = L.Grid((C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(res, res, res), 0)
    nbytes = C.c_size_t(0)
    L.check(lib.nrf_mesh_workspace_bytes(C.byref(grid), C.byref(nbytes)), lib)
    ws = torch.empty((nbytes.value + 3) // 4, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)

    def count():
      L.check(lib.nrf_mesh_count(flat.data_ptr(), C.byref(grid), thr, counts.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream), lib)

    count()
    V, F = counts.tolist()
    vertices = torch.empty(V, 3, device=dev)
    cell = torch.empty(V, dtype=torch.int32, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)

    def emit():
      L.check(lib.nrf_mesh_emit(flat.data_ptr(), C.byref(grid), thr, V, F, vertices.data_ptr(), cell.data_ptr(), faces.data_ptr(), ws.data_ptr(),
                                ws.numel() * 4, stream), lib)

    emit()
    print(f'[bench_mesh] {res}^3: V {V} F {F}, timing', file=sys.stderr, flush=True)
    assert tuple(ws[:4].tolist()) == (V, F, V, F)
    ref = evaluation.extract_mesh_from_grid(sigma, origin, step, thr, lib=lib)
    assert torch.equal(ref['vertices'], vertices) and torch.equal(ref['faces'], faces)
    copy_dst = torch.empty_like(flat)
    inside = torch.empty(n, dtype=torch.bool, device=dev)
    start = vertices.clone()

    def refine():
      q = model.query_gradient(fp, vertices, use_warp=False, outputs=('sigma', 'grad_sigma'))
      L.check(lib.nrf_mesh_snap(vertices.data_ptr(), cell.data_ptr(), q['sigma'].data_ptr(), q['grad_sigma'].data_ptr(), C.byref(grid), thr, V,
                                stream), lib)

    variants = {
        'density grid': lambda: evaluation.density_grid(model, fp, lo, hi, res),
        'count': count,
        'emit': emit,
        'count + emit': lambda: (count(), emit()),
        'device copy of the grid': lambda: copy_dst.copy_(flat),
        'inside bytes': lambda: torch.gt(flat, thr, out=inside),
        'density at V points': lambda: model.query_points(fp, start, use_warp=False, outputs=('sigma',)),
        'refine step': refine,
    }
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
    cells = (res - 1) ** 3
    # what the passes must move: count reads the grid and writes a mask byte per cell; emit reads the mask (twice: vertices, faces),
    # writes the map, and writes the mesh; the corner re-reads of active cells and the map reads of the quads come on top
    b_count = 4 * n + cells
    b_emit = 2 * cells + 4 * cells + 16 * V + 12 * F
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9
    copy_gbs = gbs(2 * 4 * n, med['device copy of the grid'][0])
    g = rec['grids'][str(res)] = {
        'points': n, 'cells': cells, 'threshold': thr, 'V': V, 'F': F, 'workspace_bytes': nbytes.value,
        'ms': {k: list(v) for k, v in med.items()}, 'runs': {k: len(v) for k, v in times.items()},
        'bytes': {'count': b_count, 'emit': b_emit}, 'copy_GBps': copy_gbs,
        'count_GBps': gbs(b_count, med['count'][0]), 'emit_GBps': gbs(b_emit, med['emit'][0]),
        'share_of_density_grid': med['count + emit'][0] / med['density grid'][0],
        'refine_in_density_queries': med['refine step'][0] / med['density at V points'][0]}
    print(f'\n## {res}^3 grid: {n} samples, {cells} cells, threshold {thr:.6g} (the median), V = {V}, F = {F} ({device}, csrc_sha16 {rec["csrc_sha16"]})\n')
    print('| what | runs | ms (10th .. 90th percentile) |')
    print('|---|---|---|')
    for k, (m, l, h) in med.items():
      print(f'| {k} | {len(times[k])} | {m:.3f} ({l:.3f} .. {h:.3f}) |')
    print(f'\n- count + emit is {100 * g["share_of_density_grid"]:.2f} % of the density grid of the same run.')
    print(f'- count must move {b_count / 1e6:.1f} MB: {g["count_GBps"]:.0f} GB/s; emit {b_emit / 1e6:.1f} MB: {g["emit_GBps"]:.0f} GB/s; '
          f'the plain copy of the grid (read + write, {8 * n / 1e6:.1f} MB) reaches {copy_gbs:.0f} GB/s.')
    print(f'- a refine step costs {g["refine_in_density_queries"]:.2f} density-only queries over the same {V} points.', flush=True)
  if args.json:
    with open(args.json, 'w') as f:
      json.dump(rec, f, indent=1)


if __name__ == '__main__':
  main()
