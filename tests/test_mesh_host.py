"""Mesh extraction on the host (no GPU): NRF_HAS_MESH next to an unchanged NRF_VERSION, the exports, every refusal the four entries
decide before any HIP call (one assertion per rule, the offending name in nrf_last_error; stand-in pointers, nothing is touched),
the workspace size, the recorded side plan sizes, evaluation.extract_mesh's calls against a recorder library, and the NumPy
restatement of the definition (tests/mesh_reference.py) on the check grids with the counts the definition's author quotes."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import mesh_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NRF_E_NULL, NRF_E_SHAPE, NRF_E_WORKSPACE = -1, -2, -5   # include/nerfies_amd.h
ENTRIES = ('nrf_mesh_workspace_bytes', 'nrf_mesh_count', 'nrf_mesh_emit', 'nrf_mesh_snap')


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()
  return L.load_library()


def test_macros_and_status_match_the_compiled_header(tmp_path, lib):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  assert cc is not None, 'no C compiler'
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(nrf_mesh_status));']
  for fname, _ in L.MeshStatus._fields_:
    lines.append(f'  printf("{fname} %zu\\n", offsetof(nrf_mesh_status, {fname}));')
  lines += ['  printf("NRF_HAS_MESH %d\\n", NRF_HAS_MESH);', '  printf("NRF_VERSION %d\\n", NRF_VERSION);',
            '  printf("NRF_MESH_MAX_CELLS %d\\n", NRF_MESH_MAX_CELLS);', '  printf("grid %zu\\n", sizeof(nrf_grid));', '  return 0;', '}']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    k, v = line.split()
    got[k] = int(v)
  assert got['NRF_HAS_MESH'] == 1
  assert got['NRF_VERSION'] == 660 == lib.nrf_version() == L.NRF_VERSION
  assert got['NRF_MESH_MAX_CELLS'] == L.NRF_MESH_MAX_CELLS == 1 << 28
  assert 6 * got['NRF_MESH_MAX_CELLS'] < 1 << 31                 # what sized it: six triangles per cell at most, indexed in int32
  assert got['size'] == C.sizeof(L.MeshStatus) == 16 and got['grid'] == C.sizeof(L.Grid) == 40
  for fname, _ in L.MeshStatus._fields_:
    assert got[fname] == getattr(L.MeshStatus, fname).offset, fname
  for name in ENTRIES:
    assert name in L.EXPORTS and hasattr(lib, name), name


class _Call:
  """The four entries with stand-in buffers: nothing is touched before a refusal."""

  def __init__(self, lib):
    from nerfies_amd import lib as L
    self.L, self.lib = L, lib
    self.buf = (C.c_float * 64)()
    self.p = C.cast(self.buf, C.c_void_p)

  def grid(self, dims=(5, 3, 7)):
    return self.L.Grid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(*dims), 0)

  def _g(self, grid, dims):
    return None if grid is None else C.byref(self.grid(dims))

  def pick(self, v):
    return self.p if v == 'p' else v

  def size(self, dims=(5, 3, 7), grid='g', out='n'):
    n = C.c_size_t(0)
    rc = self.lib.nrf_mesh_workspace_bytes(self._g(grid, dims), C.byref(n) if out == 'n' else None)
    return rc, n.value

  def count(self, sigma='p', dims=(5, 3, 7), grid='g', thr=0.5, counts='p', ws='p', nbytes=1 << 40):
    return self.lib.nrf_mesh_count(self.pick(sigma), self._g(grid, dims), thr, self.pick(counts), self.pick(ws), nbytes, None)

  def emit(self, sigma='p', dims=(5, 3, 7), grid='g', thr=0.5, mv=4, mt=4, vertices='p', cell='p', tris='p', ws='p', nbytes=1 << 40):
    return self.lib.nrf_mesh_emit(self.pick(sigma), self._g(grid, dims), thr, mv, mt, self.pick(vertices), self.pick(cell), self.pick(tris),
                                  self.pick(ws), nbytes, None)

  def snap(self, vertices='p', cell='p', sigma_at='p', grad_at='p', dims=(5, 3, 7), grid='g', thr=0.5, n=4):
    return self.lib.nrf_mesh_snap(self.pick(vertices), self.pick(cell), self.pick(sigma_at), self.pick(grad_at), self._g(grid, dims), thr, n,
                                  None)

  def err(self):
    return self.lib.nrf_last_error()


def test_null_arguments(lib):
  c = _Call(lib)
  assert c.size(grid=None)[0] == NRF_E_NULL and b'nrf_mesh_workspace_bytes: grid' in c.err()
  assert c.size(out=None)[0] == NRF_E_NULL and b'nrf_mesh_workspace_bytes: bytes' in c.err()
  assert c.count(sigma=None) == NRF_E_NULL and b'nrf_mesh_count: sigma' in c.err()
  assert c.count(grid=None) == NRF_E_NULL and b'nrf_mesh_count: grid' in c.err()
  assert c.count(counts=None) == NRF_E_NULL and b'nrf_mesh_count: counts' in c.err()
  assert c.count(ws=None) == NRF_E_NULL and b'nrf_mesh_count: workspace' in c.err()
  assert c.emit(sigma=None) == NRF_E_NULL and b'nrf_mesh_emit: sigma' in c.err()
  assert c.emit(grid=None) == NRF_E_NULL and b'nrf_mesh_emit: grid' in c.err()
  assert c.emit(vertices=None) == NRF_E_NULL and b'nrf_mesh_emit: vertices' in c.err()
  assert c.emit(cell=None) == NRF_E_NULL and b'nrf_mesh_emit: vertex_cell' in c.err()
  assert c.emit(tris=None) == NRF_E_NULL and b'nrf_mesh_emit: triangles' in c.err()
  assert c.emit(ws=None) == NRF_E_NULL and b'nrf_mesh_emit: workspace' in c.err()
  assert c.snap(vertices=None) == NRF_E_NULL and b'nrf_mesh_snap: vertices' in c.err()
  assert c.snap(cell=None) == NRF_E_NULL and b'nrf_mesh_snap: vertex_cell' in c.err()
  assert c.snap(sigma_at=None) == NRF_E_NULL and b'nrf_mesh_snap: sigma_at' in c.err()
  assert c.snap(grad_at=None) == NRF_E_NULL and b'nrf_mesh_snap: grad_at' in c.err()
  assert c.snap(grid=None) == NRF_E_NULL and b'nrf_mesh_snap: grid' in c.err()
  # a buffer of capacity 0 may be NULL (the workspace rule is the next one met), and an empty snap is a no-op
  assert c.emit(mv=0, mt=0, vertices=None, cell=None, tris=None, nbytes=0) == NRF_E_WORKSPACE
  assert c.snap(n=0, vertices=None, cell=None, sigma_at=None, grad_at=None) == 0


def test_shape_rules(lib):
  c = _Call(lib)
  for axis in range(3):
    dims = [5, 3, 7]
    dims[axis] = 1
    name = b'dims[%d]' % axis
    assert c.size(dims=dims)[0] == NRF_E_SHAPE and b'nrf_mesh_workspace_bytes' in c.err() and name in c.err()
    assert c.count(dims=dims) == NRF_E_SHAPE and b'nrf_mesh_count' in c.err() and name in c.err()
    assert c.emit(dims=dims) == NRF_E_SHAPE and b'nrf_mesh_emit' in c.err() and name in c.err()
    assert c.snap(dims=dims) == NRF_E_SHAPE and b'nrf_mesh_snap' in c.err() and name in c.err()
  assert c.count(dims=(0, 3, 7)) == NRF_E_SHAPE and c.count(dims=(5, -4, 7)) == NRF_E_SHAPE
  # 2^28 cells pass the cell rule (the workspace one refuses them here); one more row of cells does not
  full = ((1 << 14) + 1, (1 << 14) + 1, 2)
  assert c.count(dims=full, nbytes=0) == NRF_E_WORKSPACE
  assert c.size(dims=full)[0] == 0
  for over in (((1 << 14) + 2, (1 << 14) + 1, 2), ((1 << 14) + 1, (1 << 14) + 1, 3), (1 << 30, 1 << 30, 1 << 30)):
    assert c.size(dims=over)[0] == NRF_E_SHAPE and b'nrf_mesh_workspace_bytes' in c.err() and b'NRF_MESH_MAX_CELLS' in c.err()
    assert c.count(dims=over) == NRF_E_SHAPE and b'nrf_mesh_count' in c.err() and b'NRF_MESH_MAX_CELLS' in c.err()
    assert c.emit(dims=over) == NRF_E_SHAPE and b'nrf_mesh_emit' in c.err() and b'NRF_MESH_MAX_CELLS' in c.err()
    assert c.snap(dims=over) == NRF_E_SHAPE and b'nrf_mesh_snap' in c.err() and b'NRF_MESH_MAX_CELLS' in c.err()
  for bad in (float('nan'), float('inf'), float('-inf')):
    assert c.count(thr=bad) == NRF_E_SHAPE and b'nrf_mesh_count' in c.err() and b'threshold' in c.err()
    assert c.emit(thr=bad) == NRF_E_SHAPE and b'nrf_mesh_emit' in c.err() and b'threshold' in c.err()
    assert c.snap(thr=bad) == NRF_E_SHAPE and b'nrf_mesh_snap' in c.err() and b'threshold' in c.err()
  assert c.emit(mv=-1) == NRF_E_SHAPE and b'nrf_mesh_emit' in c.err() and b'max_vertices' in c.err()
  assert c.emit(mt=-1) == NRF_E_SHAPE and b'nrf_mesh_emit' in c.err() and b'max_triangles' in c.err()
  assert c.snap(n=-1) == NRF_E_SHAPE and b'nrf_mesh_snap' in c.err() and b'num_vertices' in c.err()


def test_workspace_size_and_short_workspaces(lib):
  c = _Call(lib)
  rc, base = c.size()
  assert rc == 0 and base > 0 and c.size() == (0, base)          # equal grids, equal sizes
  assert c.count(nbytes=base - 1) == NRF_E_WORKSPACE and b'nrf_mesh_count' in c.err() and b'nrf_mesh_workspace_bytes' in c.err()
  assert c.emit(nbytes=base - 1) == NRF_E_WORKSPACE and b'nrf_mesh_emit' in c.err() and b'nrf_mesh_workspace_bytes' in c.err()
  # a workspace that is not 16-byte aligned is NRF_E_SHAPE here; the components and raster entries answer NRF_E_WORKSPACE to the same
  # thing (their host tests pin that).  The codes are part of the ABI as they stand.
  off = C.c_void_p(((c.p.value + 15) & ~15) + 4)
  assert c.count(ws=off) == NRF_E_SHAPE and b'nrf_mesh_count' in c.err() and b'16-byte aligned' in c.err()
  assert c.emit(ws=off) == NRF_E_SHAPE and b'nrf_mesh_emit' in c.err() and b'16-byte aligned' in c.err()
  # origin, step and threshold play no part
  g = c.grid()
  g.origin[0], g.step[2] = 3.0, 0.25
  n = C.c_size_t(0)
  assert lib.nrf_mesh_workspace_bytes(C.byref(g), C.byref(n)) == 0 and n.value == base
  # non-decreasing in each dimension
  for axis in range(3):
    last = 0
    for v in (2, 3, 4, 7, 8, 9, 33, 64, 65, 129, 300):
      dims = [6, 5, 4]
      dims[axis] = v
      rc, size = c.size(dims=dims)
      assert rc == 0 and size >= last, (axis, v, size, last)
      last = size
  # a corner mask and a map entry per cell: 5 bytes, and change
  rc, big = c.size(dims=(257, 257, 257))
  assert rc == 0 and 5 * 256 ** 3 <= big <= 5.1 * 256 ** 3


def test_recorded_side_plan_sizes_still_hold(lib):
  spec = importlib.util.spec_from_file_location('make_side_plan_sizes', os.path.join(GOLDEN, 'make_side_plan_sizes.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  c = _Call(lib)
  assert c.size()[0] == 0                                        # a mesh workspace sized in between moves nothing
  with open(os.path.join(GOLDEN, 'side_plan_sizes.json')) as fp:
    assert mod.sizes(lib) == json.load(fp)['sizes']


def test_extract_mesh_calls(lib, monkeypatch):
  """density_grid's chunks, then count and emit on the same grid, workspace and threshold, then per refine step one gradient query
  at the vertices and one snap, a last gradient query for the normals and the colour query along the fixed view direction.  The
  recorders never follow a pointer, so everything runs on CPU tensors (the model's own device rule is lifted for that)."""
  import torch
  from nerfies_amd import evaluation, lib as L
  V, F = 37, 70
  def peek(c):   # host memory here: what the colour query's group holds while the call runs
    if c['fn'] == 'points':
      c['view'] = list((C.c_float * 3).from_address(c['viewdirs']))
      c['appearance'], c['camera'] = (C.c_int32.from_address(c[k]).value for k in ('appearance_ids', 'camera_ids'))

  rec = H.RecordingLib(lib, ['nrf_query_grid', 'nrf_query_points', 'nrf_query_points_grad', *ENTRIES[1:]], found=(V, F), peek=peek)
  model, fp = H.cpu_field_model(rec, use_appearance_metadata=True, use_camera_metadata=True)
  H.lift_device_rule(monkeypatch)
  res, lo, hi = (5, 3, 7), (-1.0, 0.0, 1.0), (1.0, 3.0, 2.0)
  mesh = evaluation.extract_mesh(model, fp, lo, hi, res, 0.75, level='coarse', warp_id=2, appearance_id=1, camera_id=1, refine_steps=2,
                                 colors=False, chunk=32)
  assert set(mesh) == {'vertices', 'faces', 'normals', 'sigma'}
  assert tuple(mesh['vertices'].shape) == (V, 3) and tuple(mesh['faces'].shape) == (F, 3) and mesh['faces'].dtype == torch.int32
  assert tuple(mesh['normals'].shape) == (V, 3) and tuple(mesh['sigma'].shape) == (V,)
  fns = [c['fn'] for c in rec.calls]
  assert fns == ['grid'] * 4 + ['count', 'emit', 'grad', 'snap', 'grad', 'snap', 'grad']
  grids = rec.calls[:4]
  assert [(c['first'], c['count']) for c in grids] == evaluation.grid_chunks(105, 32)
  want_step, want_origin = (0.4, 1.0, 1.0 / 7), (-0.8, 0.5, 1.0 + 0.5 / 7)     # density_grid's voxel centres are the samples
  count, emit = rec.calls[4], rec.calls[5]
  for c in grids + [count, emit, rec.calls[7], rec.calls[9]]:
    assert c['dims'] == res and c['step'] == pytest.approx(want_step) and c['origin'] == pytest.approx(want_origin)
  assert all(c['level'] == 0 and c['flags'] == 0 and c['warp_ids'] and c['rgb'] is None for c in grids)
  assert count['sigma'] == grids[0]['sigma'] == emit['sigma']                  # the grid tensor itself, not a copy
  assert count['thr'] == emit['thr'] == 0.75 and (count['ws'], count['nbytes']) == (emit['ws'], emit['nbytes'])
  n = C.c_size_t(0)
  assert lib.nrf_mesh_workspace_bytes(C.byref(_Call(lib).grid(res)), C.byref(n)) == 0 and count['nbytes'] >= n.value
  assert (emit['mv'], emit['mt']) == (V, F) and emit['vertices'] == mesh['vertices'].data_ptr() and emit['tris'] == mesh['faces'].data_ptr()
  for grad, snap in ((rec.calls[6], rec.calls[7]), (rec.calls[8], rec.calls[9])):
    assert grad['points'] == mesh['vertices'].data_ptr() and grad['S'] == V and grad['num_rays'] == 1 and grad['level'] == 0
    assert grad['sigma'] and grad['grad'] and grad['normals'] is None and grad['warp_ids'] and grad['flags'] == 0
    assert snap['vertices'] == mesh['vertices'].data_ptr() and snap['cell'] == emit['cell'] and snap['n'] == V and snap['thr'] == 0.75
    assert snap['sigma_at'] == grad['sigma'] and snap['grad_at'] == grad['grad']
  last = rec.calls[10]
  assert last['points'] == mesh['vertices'].data_ptr() and last['normals'] == mesh['normals'].data_ptr() and last['sigma'] == mesh['sigma'].data_ptr()
  assert last['grad'] is None

  # the canonical volume, no refinement, colours: NRF_FLAG_NO_WARP everywhere, no snap, one colour query in chunks of `chunk`
  rec.calls.clear()
  mesh = evaluation.extract_mesh(model, fp, (0, 0, 0), (1, 1, 1), 4, 0.5, appearance_id=1, camera_id=0, refine_steps=0, chunk=20)
  assert [c['fn'] for c in rec.calls] == ['grid'] * 4 + ['count', 'emit', 'grad', 'points', 'points']
  assert all(c['flags'] == L.NRF_FLAG_NO_WARP and c['warp_ids'] is None for c in rec.calls if c['fn'] in ('grid', 'grad'))
  assert all(c['level'] == 1 for c in rec.calls if c['fn'] in ('grid', 'grad'))
  assert all(c['appearance_ids'] is None for c in rec.calls if c['fn'] in ('grid', 'grad'))   # not a use_alpha_condition model
  pts = [c for c in rec.calls if c['fn'] == 'points']
  assert [(c['points'] - mesh['vertices'].data_ptr(), c['S']) for c in pts] == [(0, 20), (240, 17)]
  for c in pts:
    assert c['view'] == list(evaluation.MESH_VIEW_DIRECTION) and (c['warp_ids'], c['appearance'], c['camera']) == (None, 1, 0)
    assert c['rgb'] and c['sigma'] is None and c['warped'] is None and c['level'] == 1 and c['flags'] == L.NRF_FLAG_NO_WARP
    assert c['num_rays'] == 1
  assert tuple(mesh['rgb'].shape) == (V, 3) and set(mesh) == {'vertices', 'faces', 'normals', 'sigma', 'rgb'}

  # an empty mesh: nothing is queried behind the emit
  rec.calls.clear()
  rec.found = (0, 0)
  mesh = evaluation.extract_mesh(model, fp, (0, 0, 0), (1, 1, 1), 4, 0.5, refine_steps=3)
  assert [c['fn'] for c in rec.calls] == ['grid', 'count', 'emit']
  assert rec.calls[2]['vertices'] is None and rec.calls[2]['tris'] is None and (rec.calls[2]['mv'], rec.calls[2]['mt']) == (0, 0)
  assert {k: tuple(v.shape) for k, v in mesh.items()} == {'vertices': (0, 3), 'faces': (0, 3), 'normals': (0, 3), 'sigma': (0,), 'rgb': (0, 3)}


def test_extract_mesh_from_grid_takes_any_memory_order(lib):
  import torch
  from nerfies_amd import evaluation
  rec = H.RecordingLib(lib, ENTRIES[1:])
  native = torch.zeros(7, 3, 5).permute(2, 1, 0)                  # (5, 3, 7), x fastest in memory: what density_grid returns
  evaluation.extract_mesh_from_grid(native, (0, 0, 0), (1, 1, 1), 0.5, lib=rec)
  assert rec.calls[0]['sigma'] == native.data_ptr() and rec.calls[0]['dims'] == (5, 3, 7)
  rec.calls.clear()
  other = torch.zeros(5, 3, 7)                                    # z fastest: copied once
  evaluation.extract_mesh_from_grid(other, (0, 0, 0), (1, 1, 1), 0.5, lib=rec)
  assert rec.calls[0]['sigma'] != other.data_ptr() and rec.calls[0]['dims'] == (5, 3, 7)
  with pytest.raises(ValueError, match='sigma'):
    evaluation.extract_mesh_from_grid(torch.zeros(5, 3), (0, 0, 0), (1, 1, 1), 0.5, lib=rec)


@pytest.mark.parametrize('name', sorted(M.CHECK_GRIDS))
def test_reference_invariants_on_the_check_grids(name):
  sigma, origin, step, thr = M.CHECK_GRIDS[name]()
  v, cells, f = M.surface_nets(sigma, origin, step, thr)
  V, F, chi = M.EXPECTED[name]
  assert (len(v), len(f)) == (V, F) and len(cells) == V
  assert (np.diff(cells) > 0).all()                              # vertices in cell order
  if F == 0:
    return
  assert f.min() >= 0 and f.max() < V
  closed, opposite, _ = M.edge_report(f)
  assert closed and opposite
  assert M.euler_characteristic(V, f) == chi
  assert M.signed_volume(v, f) > 0
  if name == 'sphere':
    r = np.sqrt(((v.astype(np.float64) - np.asarray(M.CENTRE)) ** 2).sum(-1))
    assert np.abs(r - 0.6).max() <= 0.5 * np.sqrt(sum(s * s for s in step))
    assert np.abs(r - 0.6).max() <= 0.0195                       # the figure quoted with the definition: at most 0.019


def test_reference_snap_formula_by_hand():
  """One vertex whose step is exact in float32: x - (sigma - thr) / |g|^2 g, then the clamp."""
  v = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]], dtype=np.float32)
  g = np.array([[2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 4.0, 0.0]], dtype=np.float32)
  s = np.array([1.5, 1.5, 9.0], dtype=np.float32)
  out = M.snap(v, np.zeros(3, dtype=np.int32), s, g, (0, 0, 0), (1, 1, 1), (3, 3, 3), 1.0)
  assert out.tolist() == [[0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.0, 0.5]]   # a plain step; s = 0: unchanged; cut by the clamp
