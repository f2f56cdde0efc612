"""Mesh extraction on the GPU (nrf_mesh_count / nrf_mesh_emit / nrf_mesh_snap, evaluation.extract_mesh, export_density --mesh).

The kernels against tests/mesh_reference.py (the header's definition restated in NumPy float32): faces and vertex cells equal, vertices
bit for bit -- the operation order is the contract and nothing is contracted.  The only conditions that are not bitwise are the
analytic sphere bound (every vertex within half a voxel diagonal of the radius) and the median condition of the refinement below.

Median condition.  With refine_steps=2 the median over vertices of |sigma(v) - threshold| must not exceed the one at refine_steps=0.
That is a property the definition has to have by itself, so it was checked without any GPU before it went in here: for the two
models below (test_gpu_field_gradient.py's b_no_condition and g_se3 with warp id 2, trained_like, seed 14), box LO..HI, resolution
(9, 8, 7), level fine and the threshold set to the median of the grid, the float64 oracle evaluated the grid at the float32 voxel
centres, tests/mesh_reference.py meshed it, and two Newton steps x -= (sigma - thr) / |g|^2 g with the oracle's autograd gradient,
each clamped to the vertex's cell, were run in float64 on the CPU.  Median |sigma - thr| per step: b_no_condition 0.0289 -> 0.0071
-> 0.0011 (274 vertices), g_se3 0.0236 -> 0.0064 -> 0.00086 (320 vertices).  It drops by a factor of 25; the first seed and threshold
tried were kept."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import helpers as H
import mesh_reference as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI, RES = (-0.9, -0.35, 0.1), (0.6, 0.55, 1.15), (9, 8, 7)
_REF = {}


def _random(dims, seed):
  return np.random.RandomState(seed).rand(*dims).astype(np.float32), (0.25, -1.0, 3.0), (0.5, 0.125, 0.3), 0.5


def _special():
  s, origin, step, thr = _random((7, 6, 5), 3)
  s[2, 3, 1] = np.nan
  s[4, 2, 3] = np.inf
  s[3, 3, 2] = thr            # exactly the threshold: outside
  s[5, 1, 1] = -np.inf
  return s, origin, step, thr


GRIDS = dict(M.CHECK_GRIDS)
GRIDS.update({
    'random_6_5_4': lambda: _random((6, 5, 4), 0),
    'random_131_5_3': lambda: _random((131, 5, 3), 1),     # 1040 cells: rows straddle waves, two workgroups
    'random_67_9_5': lambda: _random((67, 9, 5), 2),       # 2112 cells: three workgroups
    'all_outside': lambda: (np.zeros((5, 4, 3), np.float32), (0, 0, 0), (1, 1, 1), 0.5),
    'all_inside': lambda: (np.ones((5, 4, 3), np.float32), (0, 0, 0), (1, 1, 1), 0.5),
    'nan_inf_equal': _special,
})


def reference(name):
  """(grid, origin, step, threshold, reference vertices, cells, faces): CPU only, computed once, never changed."""
  if name not in _REF:
    s, origin, step, thr = GRIDS[name]()
    _REF[name] = (s, origin, step, thr) + M.surface_nets(s, origin, step, thr)
  return _REF[name]


def _bits(t):
  return t.contiguous().view(torch.int32)


def _gpu_mesh(name):
  from nerfies_amd import evaluation
  s, origin, step, thr = reference(name)[:4]
  return evaluation.extract_mesh_from_grid(torch.from_numpy(s).to(H.DEV), origin, step, thr)


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_kernels_match_the_reference(name):
  _, _, _, _, v, cells, f = reference(name)
  got = _gpu_mesh(name)
  assert tuple(got['vertices'].shape) == (len(v), 3) and tuple(got['faces'].shape) == (len(f), 3), (name, got['vertices'].shape, got['faces'].shape)
  assert got['faces'].dtype == torch.int32 and got['vertex_cell'].dtype == torch.int32 and got['vertices'].dtype == torch.float32
  assert torch.equal(got['faces'].cpu(), torch.from_numpy(f)), name
  assert torch.equal(got['vertex_cell'].cpu(), torch.from_numpy(cells)), name
  assert torch.equal(_bits(got['vertices'].cpu()), _bits(torch.from_numpy(v))), (name, float((got['vertices'].cpu() - torch.from_numpy(v)).abs().max()))
  if name in ('all_outside', 'all_inside'):
    assert len(v) == 0 and len(f) == 0
  if name.startswith('random_1') or name.startswith('random_67'):
    assert len(v) > 1024 // 2                                    # a real surface in every workgroup


@pytest.mark.parametrize('name', ['sphere', 'torus'])
def test_invariants_of_the_gpu_mesh(name):
  _, _, step, _ = reference(name)[:4]
  got = _gpu_mesh(name)
  v, f = got['vertices'].cpu().numpy(), got['faces'].cpu().numpy()
  V, F, chi = M.EXPECTED[name]
  assert (len(v), len(f)) == (V, F)
  closed, opposite, _ = M.edge_report(f)
  assert closed and opposite
  assert M.euler_characteristic(len(v), f) == chi
  assert M.signed_volume(v, f) > 0
  if name == 'sphere':
    r = np.sqrt(((v.astype(np.float64) - np.asarray(M.CENTRE)) ** 2).sum(-1))
    bound = 0.5 * np.sqrt(sum(s * s for s in step))
    print(f'[mesh sphere] max |r - 0.6| {np.abs(r - 0.6).max():.4f}, half voxel diagonal {bound:.4f}')
    assert np.abs(r - 0.6).max() <= bound


class _Raw:
  """The entries themselves on device tensors, with `pad` canary elements behind every output."""
  CANARY_I, CANARY_F = -77777, -12345.5

  def __init__(self, name):
    from nerfies_amd import lib as L
    self.L, self.lib = L, L.load_library()
    s, origin, step, thr = reference(name)[:4]
    self.thr = float(thr)
    self.sigma = torch.from_numpy(np.ascontiguousarray(s.transpose(2, 1, 0))).to(H.DEV).reshape(-1)
    self.grid = L.Grid((C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*s.shape), 0)
    n = C.c_size_t(0)
    L.check(self.lib.nrf_mesh_workspace_bytes(C.byref(self.grid), C.byref(n)), self.lib)
    self.ws = torch.zeros((n.value + 3) // 4, dtype=torch.int32, device=H.DEV)
    self.stream = torch.cuda.current_stream(torch.device(H.DEV)).cuda_stream

  def count(self):
    counts = torch.full((2,), -1, dtype=torch.int32, device=H.DEV)
    self.L.check(self.lib.nrf_mesh_count(self.sigma.data_ptr(), C.byref(self.grid), self.thr, counts.data_ptr(), self.ws.data_ptr(),
                                         self.ws.numel() * 4, self.stream), self.lib)
    return tuple(counts.tolist())

  def emit(self, V, F, max_v, max_t, pad=64):
    v = torch.full((V + pad, 3), self.CANARY_F, dtype=torch.float32, device=H.DEV)
    c = torch.full((V + pad,), self.CANARY_I, dtype=torch.int32, device=H.DEV)
    t = torch.full((F + pad, 3), self.CANARY_I, dtype=torch.int32, device=H.DEV)
    self.L.check(self.lib.nrf_mesh_emit(self.sigma.data_ptr(), C.byref(self.grid), self.thr, max_v, max_t, v.data_ptr(), c.data_ptr(),
                                        t.data_ptr(), self.ws.data_ptr(), self.ws.numel() * 4, self.stream), self.lib)
    return v, c, t, tuple(self.ws[:4].tolist())


def test_two_runs_agree_bit_for_bit():
  for name in ('torus', 'random_67_9_5'):
    runs = []
    for _ in range(2):
      raw = _Raw(name)
      V, F = raw.count()
      v, c, t, status = raw.emit(V, F, V, F)
      assert status == (V, F, V, F)
      runs.append((v, c, t))
    for a, b in zip(*runs):
      assert torch.equal(_bits(a), _bits(b)), name
    assert (V, F) == (len(reference(name)[4]), len(reference(name)[6]))


def test_a_short_capacity_writes_nothing_and_is_reported():
  name = 'random_67_9_5'
  _, _, _, _, rv, rc, rf = reference(name)
  raw = _Raw(name)
  V, F = raw.count()
  assert (V, F) == (len(rv), len(rf)) and V > 1 and F > 1
  for max_v, max_t in ((V - 1, F), (V, F - 1), (0, 0)):
    v, c, t, status = raw.emit(V, F, max_v, max_t)
    # nrf_mesh_status: the totals stand, emitted_* are 0 -- and nothing at all was written, at or past the capacity or before it
    assert status == (V, F, 0, 0), (max_v, max_t, status)
    assert bool((v == raw.CANARY_F).all()) and bool((c == raw.CANARY_I).all()) and bool((t == raw.CANARY_I).all()), (max_v, max_t)
  # the exact capacities: the whole mesh, and the canaries behind it intact
  v, c, t, status = raw.emit(V, F, V, F)
  assert status == (V, F, V, F)
  assert torch.equal(_bits(v[:V].cpu()), _bits(torch.from_numpy(rv))) and torch.equal(c[:V].cpu(), torch.from_numpy(rc))
  assert torch.equal(t[:F].cpu(), torch.from_numpy(rf))
  assert bool((v[V:] == raw.CANARY_F).all()) and bool((c[V:] == raw.CANARY_I).all()) and bool((t[F:] == raw.CANARY_I).all())
  # larger capacities than needed change nothing
  v2, c2, t2, status = raw.emit(V, F, V + 10, F + 10)
  assert status == (V, F, V, F) and torch.equal(_bits(v2), _bits(v)) and torch.equal(t2, t)


def test_snap_is_the_documented_formula():
  from nerfies_amd import lib as L
  lib = L.load_library()
  dims, origin, step, thr = (5, 4, 3), (0.25, -1.0, 3.0), (0.5, 0.125, 0.3), 0.75
  rs = np.random.RandomState(7)
  n = 96
  ncells = 4 * 3 * 2
  cells = rs.randint(0, ncells, n).astype(np.int32)
  ci = np.stack([cells % 4, (cells // 4) % 3, cells // 12], -1)
  v = (np.float32(origin) + (ci + rs.rand(n, 3)).astype(np.float32) * np.float32(step)).astype(np.float32)
  g = rs.randn(n, 3).astype(np.float32)
  s = (thr + 0.05 * rs.randn(n)).astype(np.float32)
  g[0] = 0                                   # s = 0: unchanged
  g[1] = (0, -0.0, 0)
  s[2] = np.nan                              # sigma not finite: unchanged
  s[3] = np.inf
  s[4] = -np.inf
  g[5] = (np.inf, 1, 1)                      # s not finite: unchanged
  g[6] = (np.nan, 1, 1)
  g[7] = (2e19, 2e19, 1)                     # s overflows to inf: unchanged
  s[8], g[8] = thr + 50.0, (0.5, -0.25, 0.125)    # a step the clamp cuts on every axis
  s[9], g[9] = thr - 50.0, (0.5, -0.25, 0.125)
  s[10], g[10] = thr + 100.0, (2e-19, 0, 0)  # q overflows (s = 4e-38 is a normal number): an infinite step times a zero slope
  s[11], g[11] = thr + 1e-3, (1e-3, 2e-3, -1e-3)   # a step that stays inside on some axes only
  g[12:20] *= 1e-3
  want = M.snap(v, cells, s, g, origin, step, dims, thr)
  vt = torch.from_numpy(v).to(H.DEV)
  grid = L.Grid((C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims), 0)
  tens = [torch.from_numpy(a).to(H.DEV) for a in (cells, s, g)]
  L.check(lib.nrf_mesh_snap(vt.data_ptr(), tens[0].data_ptr(), tens[1].data_ptr(), tens[2].data_ptr(), C.byref(grid), thr, n,
                            torch.cuda.current_stream(torch.device(H.DEV)).cuda_stream), lib)
  got = vt.cpu().numpy()
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
  unchanged = [0, 1, 2, 3, 4, 5, 6, 7]
  assert np.array_equal(got[unchanged].view(np.uint32), v[unchanged].view(np.uint32))
  moved = (got != v).any(-1)
  assert moved[8] and moved[9] and moved[11] and moved[20:].all()
  lo = np.float32(origin) + ci.astype(np.float32) * np.float32(step)
  hi = np.float32(origin) + (ci + 1).astype(np.float32) * np.float32(step)
  assert ((got >= lo) & (got <= hi)).all()
  assert ((got[8] == lo[8]) | (got[8] == hi[8])).all() and ((got[9] == lo[9]) | (got[9] == hi[9])).all()   # cut on every axis


@pytest.mark.parametrize('name,warp_id', [('b_no_condition', None), ('g_se3', 2)])
def test_extract_mesh_with_a_field(name, warp_id):
  from nerfies_amd import evaluation
  from test_gpu_field_gradient import ALPHA, _model
  model, fp = _model(name)
  kw = dict(level='fine', warp_id=warp_id, warp_extra={'alpha': ALPHA})
  grid = evaluation.density_grid(model, fp, LO, HI, RES, **kw)
  thr = float(grid.reshape(-1).sort().values[grid.numel() // 2])
  step = [(h - l) / r for l, h, r in zip(LO, HI, RES)]
  origin = [l + 0.5 * s for l, s in zip(LO, step)]
  rv, rc, rf = M.surface_nets(grid.cpu().numpy(), origin, step, thr)
  assert len(rv) > 50 and len(rf) > 50                             # the median: a real surface

  m0 = evaluation.extract_mesh(model, fp, LO, HI, RES, thr, refine_steps=0, colors=False, **kw)
  assert set(m0) == {'vertices', 'faces', 'normals', 'sigma'}
  assert torch.equal(m0['faces'].cpu(), torch.from_numpy(rf))
  assert torch.equal(_bits(m0['vertices'].cpu()), _bits(torch.from_numpy(rv)))

  m2 = evaluation.extract_mesh(model, fp, LO, HI, RES, thr, refine_steps=2, **kw)
  assert set(m2) == {'vertices', 'faces', 'normals', 'sigma', 'rgb'}
  assert torch.equal(m2['faces'], m0['faces'])
  v = m2['vertices'].cpu().numpy()
  ci = np.stack([rc % (RES[0] - 1), (rc // (RES[0] - 1)) % (RES[1] - 1), rc // ((RES[0] - 1) * (RES[1] - 1))], -1)
  lo = np.float32(origin) + ci.astype(np.float32) * np.float32(step)
  hi = np.float32(origin) + (ci + 1).astype(np.float32) * np.float32(step)
  assert ((v >= lo) & (v <= hi)).all()
  assert not torch.equal(m2['vertices'], m0['vertices'])
  md = {} if warp_id is None else {'warp': torch.tensor([[warp_id]], dtype=torch.int32, device=H.DEV)}
  fresh = model.query_gradient(fp, m2['vertices'], metadata=md, warp_extra={'alpha': ALPHA}, level='fine', use_warp=warp_id is not None,
                               outputs=('sigma', 'normals'))
  assert torch.equal(_bits(m2['normals']), _bits(fresh['normals'])) and torch.equal(_bits(m2['sigma']), _bits(fresh['sigma']))
  assert tuple(m2['rgb'].shape) == (len(rv), 3) and bool(((m2['rgb'] >= 0) & (m2['rgb'] <= 1)).all())
  before = float((m0['sigma'] - thr).abs().median())
  after = float((m2['sigma'] - thr).abs().median())
  print(f'[mesh refine] {name}: V {len(rv)} F {len(rf)} threshold {thr:.6f} median |sigma - thr| {before:.3e} -> {after:.3e}')
  assert after <= before


def test_export_density_with_a_mesh_end_to_end(tmp_path):
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'scripts'))
  import train as train_driver
  import export_density
  from test_gpu_field_query import GIN
  from nerfies_amd import datasets, gin_lite as gin
  cap, exp = str(tmp_path / 'cap'), str(tmp_path / 'exp')
  datasets.write_synthetic_scene(cap, num_frames=8, size=(24, 16))
  cfg = tmp_path / 'run.gin'
  cfg.write_text(GIN)
  args = ['--base_folder', exp, '--data_dir', cap, '--gin_configs', str(cfg)]
  gin.clear_config()
  train_driver.main(args)
  for extra, name in ((['--frame', '000002'], '000002'), (['--canonical'], 'canonical')):
    common = args + extra + ['--resolution', '8']
    gin.clear_config()
    had = set(os.listdir(exp))
    plain = export_density.main(common + ['--threshold', '1e30'])
    assert not [f for f in set(os.listdir(exp)) - had if f.startswith('mesh_')]   # without --mesh: no mesh file is added,
    assert not os.path.exists(os.path.join(exp, f'mesh_{name}.ply'))
    assert set(plain) == {'npy', 'ply', 'resolution', 'num_vertices', 'bbox'}     # and the dict it always returned
    grid = np.load(plain['npy'])
    thr = float(np.sort(grid.ravel())[grid.size // 2])
    gin.clear_config()
    res = export_density.main(common + ['--threshold', repr(thr), '--mesh', '--mesh_refine', '1'])
    assert np.array_equal(np.load(res['npy']), grid)
    assert res['mesh_ply'] == os.path.join(exp, f'mesh_{name}.ply')
    V, F = res['num_mesh_vertices'], res['num_mesh_faces']
    assert V > 0 and F > 0
    blob = open(res['mesh_ply'], 'rb').read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    head = blob[:end].decode('ascii').splitlines()
    assert head[:2] == ['ply', 'format binary_little_endian 1.0']
    assert f'element vertex {V}' in head and f'element face {F}' in head
    assert [l.split()[-1] for l in head if l.startswith('property')] == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'vertex_indices']
    assert 'property list uchar int vertex_indices' in head
    assert len(blob) == end + V * (6 * 4 + 3) + F * (1 + 3 * 4)
    vert = np.frombuffer(blob, dtype=[('xyz', '<f4', 3), ('n', '<f4', 3), ('rgb', 'u1', 3)], count=V, offset=end)
    face = np.frombuffer(blob, dtype=[('n', 'u1'), ('idx', '<i4', 3)], count=F, offset=end + V * 27)
    assert (face['n'] == 3).all() and face['idx'].min() >= 0 and face['idx'].max() < V
    assert np.isfinite(vert['xyz']).all() and np.isfinite(vert['n']).all()
    lo, hi = plain['bbox']
    assert (vert['xyz'] >= lo - 1e-6).all() and (vert['xyz'] <= hi + 1e-6).all()
  gin.clear_config()
