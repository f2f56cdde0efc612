#!/usr/bin/env python
"""Mesh clean-up on one GPU, as markdown (profiles/mesh_components.md):
    python scripts/bench_mesh_components.py [--res 128 256] [--json out.json]
The workload of profiles/mesh.md: the canonical volume of the configuration-A model shape on a RES^3 grid, meshed at the MEDIAN of the
grid.  Timed, on that mesh:
    density grid            evaluation.density_grid: what the mesh starts from
    mesh count + emit       nrf_mesh_count + nrf_mesh_emit, back to back on the stream
    labelling               nrf_mesh_components (init, hook, flatten, scan, the two label kernels)
    table                   nrf_mesh_component_table with the boxes, into a table of C rows
    submesh count + emit    nrf_mesh_submesh_count + nrf_mesh_submesh_emit for the mask that keeps the largest component
    gathers                 nrf_mesh_gather_rows of the vertices (3 words), the vertex cells (1) and one more (V, 3) array
HIP events around each variant on the current stream; every variant is warmed up, then the variants ALTERNATE in one process for
--rounds rounds; median (10th .. 90th percentile).  Next to them, once and on the host clock: the CPU's labelling of the same mesh
(scipy.sparse.csgraph.connected_components where scipy imports, else the tests' NumPy reference), copy to the host not included;
the device's labels are checked against it before anything is timed."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench  # noqa: E402  (kernel_source_sha)
from nerfies_amd import evaluation, lib as L, models  # noqa: E402
from scripts.bench_field_query import CfgA, WARMUP, pct  # noqa: E402


def cpu_labels(faces, V):
  """(labels by smallest vertex, C, seconds, what ran)."""
  try:
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
  except ImportError:
    import mesh_components_reference as R
    t = time.perf_counter()
    labels, nc = R.components(faces, V)
    return labels, nc, time.perf_counter() - t, 'tests/mesh_components_reference.py (Python union-find)'
  f = faces.astype(np.int64)
  t = time.perf_counter()
  rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
  nc, lab = connected_components(sp.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)), directed=False)
  first = np.full(nc, V, dtype=np.int64)
  np.minimum.at(first, lab, np.arange(V))
  rank = np.empty(nc, dtype=np.int64)
  rank[np.argsort(first)] = np.arange(nc)
  labels = rank[lab].astype(np.int32)
  return labels, nc, time.perf_counter() - t, 'scipy.sparse.csgraph.connected_components + relabelling by smallest vertex'


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--res', type=int, nargs='+', default=[128, 256])
  ap.add_argument('--rounds', type=int, default=30, help='timed runs of every variant')
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
    mesh = evaluation.extract_mesh_from_grid(sigma, origin, step, thr, lib=lib)
    vertices, cell, faces = mesh['vertices'], mesh['vertex_cell'], mesh['faces']
    V, F = vertices.shape[0], faces.shape[0]

    def workspace(sizer, *a):
      nbytes = C.c_size_t(0)
      L.check(sizer(*a, C.byref(nbytes)), lib)
      return torch.empty((nbytes.value + 3) // 4, dtype=torch.int32, device=dev), nbytes.value

    mws, _ = workspace(lib.nrf_mesh_workspace_bytes, C.byref(grid))
    cws, cbytes = workspace(lib.nrf_mesh_components_workspace_bytes, V, F)
    sws, sbytes = workspace(lib.nrf_mesh_submesh_workspace_bytes, V, F)
    mcounts = torch.zeros(2, dtype=torch.int32, device=dev)
    mv, mc, mf = torch.empty_like(vertices), torch.empty_like(cell), torch.empty_like(faces)

    def mesh_count_emit():
      L.check(lib.nrf_mesh_count(flat.data_ptr(), C.byref(grid), thr, mcounts.data_ptr(), mws.data_ptr(), mws.numel() * 4, stream), lib)
      L.check(lib.nrf_mesh_emit(flat.data_ptr(), C.byref(grid), thr, V, F, mv.data_ptr(), mc.data_ptr(), mf.data_ptr(), mws.data_ptr(),
                                mws.numel() * 4, stream), lib)

    labels = torch.empty(V, dtype=torch.int32, device=dev)
    ccount = torch.zeros(1, dtype=torch.int32, device=dev)

    def label():
      L.check(lib.nrf_mesh_components(faces.data_ptr(), F, V, labels.data_ptr(), ccount.data_ptr(), cws.data_ptr(), cws.numel() * 4, stream), lib)

    label()
    nc = int(ccount.item())
    comp_counts = torch.empty(nc, 2, dtype=torch.int32, device=dev)
    comp_bbox = torch.empty(nc, 6, device=dev)

    def table():
      L.check(lib.nrf_mesh_component_table(faces.data_ptr(), F, vertices.data_ptr(), V, labels.data_ptr(), nc, comp_counts.data_ptr(),
                                           comp_bbox.data_ptr(), cws.data_ptr(), cws.numel() * 4, stream), lib)

    table()
    status = tuple(cws[:4].tolist())
    assert status[:3] == (nc, nc, 0), status
    print(f'[bench_mesh_components] {res}^3: V {V} F {F} C {nc}, labelling on the CPU', file=sys.stderr, flush=True)
    want, wc, cpu_s, cpu_what = cpu_labels(faces.cpu().numpy(), V)
    assert wc == nc and np.array_equal(labels.cpu().numpy(), want)
    nt = comp_counts[:, 1].tolist()
    largest = max(range(nc), key=lambda c: (nt[c], -c))
    keep = (labels == largest).to(torch.uint8)
    scounts = torch.zeros(2, dtype=torch.int32, device=dev)
    L.check(lib.nrf_mesh_submesh_count(keep.data_ptr(), V, faces.data_ptr(), F, scounts.data_ptr(), sws.data_ptr(), sws.numel() * 4, stream), lib)
    kv, kf = scounts.tolist()
    assert (kv, kf) == (comp_counts[largest, 0].item(), nt[largest])
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    faces_out = torch.empty(kf, 3, dtype=torch.int32, device=dev)

    def submesh():
      L.check(lib.nrf_mesh_submesh_count(keep.data_ptr(), V, faces.data_ptr(), F, scounts.data_ptr(), sws.data_ptr(), sws.numel() * 4, stream), lib)
      L.check(lib.nrf_mesh_submesh_emit(keep.data_ptr(), V, faces.data_ptr(), F, kv, kf, vmap.data_ptr(), faces_out.data_ptr(), sws.data_ptr(),
                                        sws.numel() * 4, stream), lib)

    submesh()
    assert tuple(sws[:4].tolist()) == (kv, kf, kv, kf)
    extra = torch.randn(V, 3, device=dev)
    outs = [torch.empty(kv, 3, device=dev), torch.empty(kv, dtype=torch.int32, device=dev), torch.empty(kv, 3, device=dev)]

    def gathers():
      for src, width, dst in ((vertices, 3, outs[0]), (cell, 1, outs[1]), (extra, 3, outs[2])):
        L.check(lib.nrf_mesh_gather_rows(src.data_ptr(), width, vmap.data_ptr(), V, dst.data_ptr(), kv, stream), lib)

    gathers()
    assert torch.equal(outs[0], vertices[keep.bool()]) and torch.equal(outs[1], cell[keep.bool()])
    variants = {
        'density grid': lambda: evaluation.density_grid(model, fp, lo, hi, res),
        'mesh count + emit': mesh_count_emit,
        'labelling': label,
        'table': table,
        'submesh count + emit': submesh,
        'gathers': gathers,
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
    clean = sum(med[k][0] for k in ('labelling', 'table', 'submesh count + emit', 'gathers'))
    sizes = sorted(nt, reverse=True)
    g = rec['grids'][str(res)] = {
        'points': n, 'threshold': thr, 'V': V, 'F': F, 'C': nc, 'largest': [kv, kf], 'triangles_of_the_largest_components': sizes[:8],
        'single_vertex_components': int((comp_counts[:, 1] == 0).sum()), 'workspace_bytes': {'components': cbytes, 'submesh': sbytes},
        'ms': {k: list(v) for k, v in med.items()}, 'runs': {k: len(v) for k, v in times.items()}, 'cpu_labelling_s': cpu_s,
        'cpu_labelling': cpu_what, 'clean_up_ms': clean, 'share_of_density_grid': clean / med['density grid'][0]}
    print(f'\n## {res}^3 grid: {n} samples, threshold {thr:.6g} (the median), V = {V}, F = {F}, C = {nc} ({device}, csrc_sha16 {rec["csrc_sha16"]})\n')
    print(f'The largest component has {kv} vertices and {kf} triangles; triangles of the largest components: {sizes[:8]}; '
          f'{g["single_vertex_components"]} components have no triangle.  Workspaces: components {cbytes} B, submesh {sbytes} B.\n')
    print('| what | runs | ms (10th .. 90th percentile) |')
    print('|---|---|---|')
    for k, (m, l, h) in med.items():
      print(f'| {k} | {len(times[k])} | {m:.3f} ({l:.3f} .. {h:.3f}) |')
    print(f'| labelling on the CPU ({cpu_what}), once | 1 | {1e3 * cpu_s:.0f} |')
    print(f'\n- labelling + table + submesh + gathers: {clean:.3f} ms, {100 * g["share_of_density_grid"]:.2f} % of the density grid of the same run '
          f'and {clean / med["mesh count + emit"][0]:.1f} x its mesh count + emit.', flush=True)
  if args.json:
    with open(args.json, 'w') as f:
      json.dump(rec, f, indent=1)


if __name__ == '__main__':
  main()
