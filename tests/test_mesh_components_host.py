"""Mesh clean-up on the host (no GPU): NRF_HAS_MESH_COMPONENTS next to an unchanged NRF_VERSION, the exports, every refusal the seven
entries decide before any HIP call (one assertion per rule, the entry's name in nrf_last_error; stand-in pointers, nothing is
touched), the workspace sizes, clean_mesh's selection rule, and the NumPy restatement of the definitions
(tests/mesh_components_reference.py) against scipy's connected components and on the fixtures with the numbers their author quotes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_components_reference as R
import mesh_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
NRF_E_NULL, NRF_E_SHAPE, NRF_E_WORKSPACE = -1, -2, -5   # include/nerfies_amd.h
ENTRIES = ('nrf_mesh_components_workspace_bytes', 'nrf_mesh_components', 'nrf_mesh_component_table', 'nrf_mesh_submesh_workspace_bytes',
           'nrf_mesh_submesh_count', 'nrf_mesh_submesh_emit', 'nrf_mesh_gather_rows')


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()
  return L.load_library()


def test_macro_status_and_exports(tmp_path, lib):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  assert cc is not None, 'no C compiler'
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(nrf_mesh_components_status));']
  for fname, _ in L.MeshComponentsStatus._fields_:
    lines.append(f'  printf("{fname} %zu\\n", offsetof(nrf_mesh_components_status, {fname}));')
  lines += ['  printf("NRF_HAS_MESH_COMPONENTS %d\\n", NRF_HAS_MESH_COMPONENTS);', '  printf("NRF_HAS_MESH %d\\n", NRF_HAS_MESH);',
            '  printf("NRF_VERSION %d\\n", NRF_VERSION);', '  return 0;', '}']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    k, v = line.split()
    got[k] = int(v)
  assert got['NRF_HAS_MESH_COMPONENTS'] == 1 and got['NRF_HAS_MESH'] == 1
  assert got['NRF_VERSION'] == 660 == lib.nrf_version() == L.NRF_VERSION
  assert got['size'] == C.sizeof(L.MeshComponentsStatus) == 16
  assert [f for f, _ in L.MeshComponentsStatus._fields_] == ['num_components', 'table_components', 'error', 'reserved']
  for fname, _ in L.MeshComponentsStatus._fields_:
    assert got[fname] == getattr(L.MeshComponentsStatus, fname).offset, fname
  for name in ENTRIES:
    assert name in L.EXPORTS and hasattr(lib, name), name


class _Call:
  """The seven entries with stand-in buffers: nothing is touched before a refusal."""

  def __init__(self, lib):
    self.lib = lib
    self.buf = (C.c_float * 64)()
    self.p = C.cast(self.buf, C.c_void_p)
    self.aligned = C.c_void_p((self.p.value + 15) // 16 * 16)

  def pick(self, v):
    return self.aligned if v == 'p' else (C.c_void_p(self.aligned.value + 4) if v == 'odd' else v)

  def size(self, which, V=7, F=9, out='n'):
    n = C.c_size_t(0)
    rc = getattr(self.lib, f'nrf_mesh_{which}_workspace_bytes')(V, F, C.byref(n) if out == 'n' else None)
    return rc, n.value

  def components(self, tris='p', F=9, V=7, labels='p', counts='p', ws='p', nbytes=1 << 40):
    return self.lib.nrf_mesh_components(self.pick(tris), F, V, self.pick(labels), self.pick(counts), self.pick(ws), nbytes, None)

  def table(self, tris='p', F=9, vertices='p', V=7, labels='p', mc=3, cc='p', box='p', ws='p', nbytes=1 << 40):
    return self.lib.nrf_mesh_component_table(self.pick(tris), F, self.pick(vertices), V, self.pick(labels), mc, self.pick(cc),
                                             self.pick(box), self.pick(ws), nbytes, None)

  def count(self, keep='p', V=7, tris='p', F=9, counts='p', ws='p', nbytes=1 << 40):
    return self.lib.nrf_mesh_submesh_count(self.pick(keep), V, self.pick(tris), F, self.pick(counts), self.pick(ws), nbytes, None)

  def emit(self, keep='p', V=7, tris='p', F=9, mv=4, mt=4, vmap='p', out='p', ws='p', nbytes=1 << 40):
    return self.lib.nrf_mesh_submesh_emit(self.pick(keep), V, self.pick(tris), F, mv, mt, self.pick(vmap), self.pick(out), self.pick(ws),
                                          nbytes, None)

  def gather(self, src='p', width=3, vmap='p', V=7, dst='p', rows=4):
    return self.lib.nrf_mesh_gather_rows(self.pick(src), width, self.pick(vmap), V, self.pick(dst), rows, None)

  def err(self):
    return self.lib.nrf_last_error()


def test_null_arguments(lib):
  c = _Call(lib)
  assert c.size('components', out=None)[0] == NRF_E_NULL and b'nrf_mesh_components_workspace_bytes: bytes' in c.err()
  assert c.size('submesh', out=None)[0] == NRF_E_NULL and b'nrf_mesh_submesh_workspace_bytes: bytes' in c.err()
  assert c.components(tris=None) == NRF_E_NULL and b'nrf_mesh_components: triangles' in c.err()
  assert c.components(labels=None) == NRF_E_NULL and b'nrf_mesh_components: vertex_component' in c.err()
  assert c.components(counts=None) == NRF_E_NULL and b'nrf_mesh_components: counts' in c.err()
  assert c.components(ws=None) == NRF_E_NULL and b'nrf_mesh_components: workspace' in c.err()
  assert c.table(tris=None) == NRF_E_NULL and b'nrf_mesh_component_table: triangles' in c.err()
  assert c.table(labels=None) == NRF_E_NULL and b'nrf_mesh_component_table: vertex_component' in c.err()
  assert c.table(cc=None) == NRF_E_NULL and b'nrf_mesh_component_table: comp_counts' in c.err()
  assert c.table(vertices=None) == NRF_E_NULL and b'nrf_mesh_component_table: vertices' in c.err()     # the two are NULL together,
  assert c.table(box=None) == NRF_E_NULL and b'nrf_mesh_component_table: comp_bbox' in c.err()         # or neither is
  assert c.table(ws=None) == NRF_E_NULL and b'nrf_mesh_component_table: workspace' in c.err()
  assert c.count(keep=None) == NRF_E_NULL and b'nrf_mesh_submesh_count: keep' in c.err()
  assert c.count(tris=None) == NRF_E_NULL and b'nrf_mesh_submesh_count: triangles' in c.err()
  assert c.count(counts=None) == NRF_E_NULL and b'nrf_mesh_submesh_count: counts' in c.err()
  assert c.count(ws=None) == NRF_E_NULL and b'nrf_mesh_submesh_count: workspace' in c.err()
  assert c.emit(keep=None) == NRF_E_NULL and b'nrf_mesh_submesh_emit: keep' in c.err()
  assert c.emit(tris=None) == NRF_E_NULL and b'nrf_mesh_submesh_emit: triangles' in c.err()
  assert c.emit(vmap=None) == NRF_E_NULL and b'nrf_mesh_submesh_emit: vertex_map' in c.err()
  assert c.emit(out=None) == NRF_E_NULL and b'nrf_mesh_submesh_emit: triangles_out' in c.err()
  assert c.emit(ws=None) == NRF_E_NULL and b'nrf_mesh_submesh_emit: workspace' in c.err()
  assert c.gather(src=None) == NRF_E_NULL and b'nrf_mesh_gather_rows: src' in c.err()
  assert c.gather(vmap=None) == NRF_E_NULL and b'nrf_mesh_gather_rows: vertex_map' in c.err()
  assert c.gather(dst=None) == NRF_E_NULL and b'nrf_mesh_gather_rows: dst' in c.err()
  # a buffer whose count or capacity is 0 may be NULL: the workspace rule is the next one met; an empty gather is a no-op
  assert c.components(tris=None, F=0, labels=None, V=0, nbytes=0) == NRF_E_WORKSPACE
  assert c.table(tris=None, F=0, vertices=None, box=None, labels=None, V=0, cc=None, mc=0, nbytes=0) == NRF_E_WORKSPACE
  assert c.table(vertices=None, box=None, nbytes=0) == NRF_E_WORKSPACE           # no boxes asked for
  assert c.count(keep=None, V=0, tris=None, F=0, nbytes=0) == NRF_E_WORKSPACE
  assert c.emit(keep=None, V=0, vmap=None, tris=None, F=0, out=None, mt=0, nbytes=0) == NRF_E_WORKSPACE
  assert c.gather(src=None, vmap=None, dst=None, V=0) == 0
  assert c.gather(dst=None, rows=0) == 0


def test_negative_counts_and_capacities(lib):
  c = _Call(lib)
  for which in ('components', 'submesh'):
    name = b'nrf_mesh_%s_workspace_bytes' % which.encode()
    assert c.size(which, V=-1)[0] == NRF_E_SHAPE and name in c.err() and b'num_vertices' in c.err()
    assert c.size(which, F=-1)[0] == NRF_E_SHAPE and name in c.err() and b'num_triangles' in c.err()
  for fn, name in ((c.components, b'nrf_mesh_components:'), (c.table, b'nrf_mesh_component_table:'), (c.count, b'nrf_mesh_submesh_count:'),
                   (c.emit, b'nrf_mesh_submesh_emit:')):
    assert fn(V=-1) == NRF_E_SHAPE and name in c.err() and b'num_vertices' in c.err()
    assert fn(F=-1) == NRF_E_SHAPE and name in c.err() and b'num_triangles' in c.err()
  assert c.table(mc=-1) == NRF_E_SHAPE and b'nrf_mesh_component_table:' in c.err() and b'max_components' in c.err()
  assert c.emit(mv=-1) == NRF_E_SHAPE and b'nrf_mesh_submesh_emit:' in c.err() and b'max_vertices' in c.err()
  assert c.emit(mt=-1) == NRF_E_SHAPE and b'nrf_mesh_submesh_emit:' in c.err() and b'max_triangles' in c.err()
  assert c.gather(V=-1) == NRF_E_SHAPE and b'nrf_mesh_gather_rows:' in c.err() and b'num_vertices' in c.err()
  assert c.gather(rows=-1) == NRF_E_SHAPE and b'nrf_mesh_gather_rows:' in c.err() and b'max_rows' in c.err()
  for width in (0, -3):
    assert c.gather(width=width) == NRF_E_SHAPE and b'nrf_mesh_gather_rows:' in c.err() and b'width' in c.err()
  assert c.gather(V=(1 << 31) - 1, width=(1 << 31) - 1) == NRF_E_SHAPE and b'nrf_mesh_gather_rows:' in c.err()


def test_workspace_rules_and_sizes(lib):
  c = _Call(lib)
  rc, comp = c.size('components')
  rc2, sub = c.size('submesh')
  assert rc == 0 and rc2 == 0 and comp >= 16 and sub >= 16
  for fn, name, need, sizer in ((c.components, b'nrf_mesh_components:', comp, b'nrf_mesh_components_workspace_bytes'),
                                (c.table, b'nrf_mesh_component_table:', comp, b'nrf_mesh_components_workspace_bytes'),
                                (c.count, b'nrf_mesh_submesh_count:', sub, b'nrf_mesh_submesh_workspace_bytes'),
                                (c.emit, b'nrf_mesh_submesh_emit:', sub, b'nrf_mesh_submesh_workspace_bytes')):
    assert fn(nbytes=need - 1) == NRF_E_WORKSPACE and name in c.err() and sizer in c.err()
    assert fn(ws='odd') == NRF_E_WORKSPACE and name in c.err() and b'16-byte aligned' in c.err()
  # empty meshes have a workspace too: the status block
  assert c.size('components', V=0, F=0) == (0, c.size('components', V=0, F=12)[1]) and c.size('components', V=0, F=0)[1] >= 16
  assert c.size('submesh', V=0, F=0)[1] >= 16
  # the triangles play no part in the components workspace; both are non-decreasing in their counts
  assert c.size('components', V=5000, F=0) == c.size('components', V=5000, F=10 ** 6)
  for which in ('components', 'submesh'):
    last = 0
    for n in (0, 1, 255, 256, 1023, 1024, 1025, 4097, 10 ** 6):
      rc, size = c.size(which, V=n, F=2 * n)
      assert rc == 0 and size >= last, (which, n)
      last = size
  # about 4 bytes per vertex and a total per workgroup of 1024; the submesh needs the totals only
  V = 4_800_000
  assert 4 * V <= c.size('components', V=V, F=2 * V)[1] <= 4.01 * V
  assert c.size('submesh', V=V, F=2 * V)[1] <= 4 * (3 * V // 1024) + 4096
  assert c.size('components', V=(1 << 31) - 1, F=(1 << 31) - 1)[0] == 0 and c.size('submesh', V=(1 << 31) - 1, F=(1 << 31) - 1)[0] == 0


def test_select_components():
  from nerfies_amd.evaluation import select_components
  nt = [52, 2688, 1036, 28, 0, 1036]
  assert select_components(nt, 'all', 1) == [0, 1, 2, 3, 5]
  assert select_components(nt, 'all', 0) == [0, 1, 2, 3, 4, 5]
  assert select_components(nt, 'largest') == [1] == select_components(nt, 1)
  assert select_components(nt, 2) == [1, 2]                     # a tie goes to the smaller id
  assert select_components(nt, 3) == [1, 2, 5]
  assert select_components(nt, 100, 30) == [0, 1, 2, 5]
  assert select_components(nt, 'largest', 10 ** 6) == [] == select_components([], 'largest')
  for bad in (0, -1, 'biggest', 1.5, True, None):
    with pytest.raises(ValueError, match='keep'):
      select_components(nt, bad)


def _scipy_labels(faces, V):
  sp = pytest.importorskip('scipy.sparse')
  from scipy.sparse.csgraph import connected_components
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  f = f[R.valid_triangles(f, V)]
  rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
  C_, lab = connected_components(sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False)
  first = np.full(C_, V, dtype=np.int64)
  np.minimum.at(first, lab, np.arange(V))                       # relabel by smallest vertex
  rank = np.empty(C_, dtype=np.int64)
  rank[np.argsort(first)] = np.arange(C_)
  return rank[lab].astype(np.int32), C_


@pytest.mark.parametrize('name', ['scene', 'random_131_5_3', 'random_67_9_5', 'serpentine_cut', 'shuffled', 'reversed', 'junk'])
def test_reference_components_against_scipy(name):
  if name in ('shuffled', 'reversed'):
    v, f = R.renumbered('serpentine_cut', 'random' if name == 'shuffled' else 'reversed', 5)
  elif name == 'junk':
    rs = np.random.RandomState(11)
    v, f = np.zeros((300, 3), np.float32), rs.randint(-20, 320, (260, 3)).astype(np.int32)   # invalid and degenerate triangles
  else:
    v, _, f = R.mesh(name)
  labels, C_ = R.components(f, len(v))
  want, wc = _scipy_labels(f, len(v))
  assert C_ == wc and np.array_equal(labels, want)


def test_fixture_numbers():
  for name, (V, F, C_) in R.EXPECTED.items():
    v, cells, f = R.mesh(name)
    labels, got, counts, box = R.labelled(name)
    assert (len(v), len(f), got) == (V, F, C_), name
    assert counts[:, 0].sum() == V and counts[:, 1].sum() == F and box.shape == (C_, 6)
    assert (box[:, :3] <= box[:, 3:]).all()
  labels, _, counts, _ = R.labelled('scene')
  assert counts[:, 0].tolist() == [28, 1346, 520, 16] and counts[:, 1].tolist() == [52, 2688, 1036, 28]
  assert [int(np.argmax(labels == c)) for c in range(4)] == [0, 28, 521, 1894]
  assert (np.diff(labels) != 0).sum() > 3                        # the ids interleave in vertex order
  counts = R.labelled('random_131_5_3')[2]
  assert ((counts[:, 0] == 1) & (counts[:, 1] == 0)).sum() == 13
  counts = R.labelled('random_67_9_5')[2]
  assert ((counts[:, 0] == 1) & (counts[:, 1] == 0)).sum() == 4
  counts = R.labelled('serpentine_cut')[2]
  assert sorted(counts[:, 1].tolist()) == [2316, 6508] and sorted(counts[:, 0].tolist()) == [1160, 3256]


def test_scene_components_are_the_balls_alone():
  """The submesh of each component equals surface_nets of that ball's grid alone, bit for bit, after the index map; each is closed
  with Euler characteristic 2."""
  v, cells, f = R.mesh('scene')
  labels = R.labelled('scene')[0]
  for cid, ball in enumerate(R.SCENE_COMPONENT_BALL):
    keep = labels == cid
    vmap, faces = R.submesh(keep, f, len(v))
    bv, bc, bf = R.mesh(f'ball{ball}')
    assert np.array_equal(R.gather_rows(v, vmap).view(np.uint32), bv.view(np.uint32)), cid
    assert np.array_equal(R.gather_rows(cells, vmap), bc) and np.array_equal(faces, bf), cid
    closed, opposite, _ = M.edge_report(faces)
    assert closed and opposite and M.euler_characteristic(len(bv), faces) == 2, cid


def test_reference_key_table_and_submesh_by_hand():
  x = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], dtype=np.float32)
  k = R.float_key(x)
  assert (np.diff(k.astype(np.int64)) > 0).all()                  # strictly increasing: -0 below +0
  assert np.array_equal(R.key_float(k).view(np.uint32), x.view(np.uint32))
  assert int(R.float_key(np.float32(np.inf))) == 0xff800000 and int(R.float_key(np.float32(-np.inf))) == 0x007fffff
  v = np.array([[0, 1, 2], [np.nan, -0.0, 5], [3, 0.0, np.nan], [np.nan, np.nan, np.nan], [7, 7, 7]], dtype=np.float32)
  f = np.array([[0, 1, 2], [2, 2, 1], [0, 1, 5], [-1, 0, 1], [4, 4, 4]], dtype=np.int32)
  labels, C_ = R.components(f, 5)
  assert labels.tolist() == [0, 0, 0, 1, 2] and C_ == 3
  counts, box = R.table(v, f, labels, C_)
  assert counts.tolist() == [[3, 2], [1, 0], [1, 1]]
  want = np.array([[0, -0.0, 2, 3, 1, 5], [np.inf] * 3 + [-np.inf] * 3, [7] * 6], dtype=np.float32)
  assert np.array_equal(box.view(np.uint32), want.view(np.uint32))
  vmap, faces = R.submesh([1, 1, 1, 0, 1], f, 5)
  assert vmap.tolist() == [0, 1, 2, -1, 3] and faces.tolist() == [[0, 1, 2], [2, 2, 1], [3, 3, 3]]
  vmap, faces = R.submesh([0, 1, 1, 1, 0], f, 5)
  assert vmap.tolist() == [-1, 0, 1, 2, -1] and faces.tolist() == [[1, 1, 0]]
