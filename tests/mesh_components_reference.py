"""Mesh clean-up in NumPy: the definitions of include/nerfies_amd.h (nrf_mesh_components / nrf_mesh_component_table /
nrf_mesh_submesh_* / nrf_mesh_gather_rows) restated with a plain union-find and boolean indexing.  Not a test: the mesh-components
tests import it.  Also their fixture meshes (tests/mesh_reference.py::surface_nets of small grids), computed once per process.

A mesh is (faces (F,3) int, V); a triangle is VALID iff its three indices are in [0, V)."""
import numpy as np

import mesh_reference as M

F32 = np.float32


def valid_triangles(faces, V):
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  return ((f >= 0) & (f < V)).all(-1)


def components(faces, V):
  """(labels (V,) int32, C): a valid triangle (a, b, c) joins a-b and b-c; ids are dense in increasing order of each component's
  smallest vertex."""
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  parent = list(range(V))

  def find(x):
    while parent[x] != x:
      x = parent[x]
    return x

  for a, b, c in f[valid_triangles(f, V)].tolist():
    for p, q in ((a, b), (b, c)):
      rp, rq = find(p), find(q)
      if rp != rq:
        parent[max(rp, rq)] = min(rp, rq)          # the root stays the smallest vertex of its tree
      for x in (p, q):                             # compress, so the long tubes stay quick
        while parent[x] != min(rp, rq):
          parent[x], x = min(rp, rq), parent[x]
  labels = np.zeros(V, dtype=np.int32)
  ids = {}
  for v in range(V):                               # increasing v: a root is met before the rest of its component
    r = find(v)
    if r not in ids:
      assert r == v
      ids[r] = len(ids)
    labels[v] = ids[r]
  return labels, len(ids)


def float_key(x):
  """The monotone uint32 key of float32 values: -0 sorts below +0."""
  u = np.asarray(x, dtype=F32).view(np.uint32)
  return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_float(k):
  k = np.asarray(k, dtype=np.uint32)
  return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def table(vertices, faces, labels, C):
  """(comp_counts (C,2) int32 = [vertices, valid triangles by first index], comp_bbox (C,6) float32 or None without vertices)."""
  V = len(labels)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  counts = np.zeros((C, 2), dtype=np.int32)
  counts[:, 0] = np.bincount(labels, minlength=C)
  first = f[valid_triangles(f, V), 0]
  counts[:, 1] = np.bincount(labels[first], minlength=C)
  if vertices is None:
    return counts, None
  v = np.asarray(vertices, dtype=F32).reshape(V, 3)
  keys = float_key(v)
  lo = np.full((C, 3), float_key(F32(np.inf)), dtype=np.uint32)
  hi = np.full((C, 3), float_key(F32(-np.inf)), dtype=np.uint32)
  for c in range(C):
    for e in range(3):
      k = keys[(labels == c) & ~np.isnan(v[:, e]), e]
      if len(k):
        lo[c, e], hi[c, e] = k.min(), k.max()
  return counts, np.concatenate([key_float(lo), key_float(hi)], -1)


def submesh(keep, faces, V):
  """(vertex_map (V,) int32, faces_out): the rank among the kept vertices or -1; the valid triangles whose vertices are all kept,
  in their order, with mapped indices."""
  keep = np.asarray(keep).reshape(V) != 0
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  vmap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
  ok = valid_triangles(f, V)
  ok[ok] = keep[f[ok]].all(-1)
  return vmap, vmap[f[ok]].astype(np.int32).reshape(-1, 3)


def gather_rows(rows, vmap):
  return np.asarray(rows)[np.asarray(vmap) >= 0]


# ---- fixtures ----
BALLS = (((12.3, 14.1, 15.2), 8.4), ((29.2, 22.7, 17.6), 5.3), ((33.1, 6.2, 5.4), 1.2), ((4.2, 30.3, 27.1), 0.9))
SCENE_DIMS = (40, 36, 33)
SCENE_ORIGIN, SCENE_STEP = (-0.9, -0.35, 0.1), (0.04, 0.025, 0.03)


def balls_grid(balls):
  """sigma = max over the balls of (r - |idx - c|), float32, on the scene's grid."""
  idx = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SCENE_DIMS], indexing='ij'), -1)
  s = np.max([r - np.sqrt(((idx - np.asarray(c)) ** 2).sum(-1)) for c, r in balls], 0)
  return s.astype(F32), SCENE_ORIGIN, SCENE_STEP, 0.0


def random_grid(dims, seed):
  return np.random.RandomState(seed).rand(*dims).astype(F32), (0.25, -1.0, 3.0), (0.5, 0.125, 0.3), 0.5


def serpentine_grid(cut=False):
  """Long thin tubes: 17 rows along x joined at alternating ends."""
  s = np.zeros((66, 35, 3), dtype=F32)
  for r, j in enumerate(range(1, 34, 2)):
    s[1:65, j, 1] = 1
    if j + 2 < 34:
      s[64 if r % 2 == 0 else 1, j + 1, 1] = 1
  if cut:
    s[30, 9, 1] = s[31, 9, 1] = 0
  return s, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.5


GRIDS = {
    'scene': lambda: balls_grid(BALLS),
    'ball0': lambda: balls_grid(BALLS[0:1]),
    'ball1': lambda: balls_grid(BALLS[1:2]),
    'ball2': lambda: balls_grid(BALLS[2:3]),
    'ball3': lambda: balls_grid(BALLS[3:4]),
    'random_131_5_3': lambda: random_grid((131, 5, 3), 1),
    'random_67_9_5': lambda: random_grid((67, 9, 5), 2),
    'serpentine': lambda: serpentine_grid(False),
    'serpentine_cut': lambda: serpentine_grid(True),
}
# (V, F, C) of every fixture, computed on the CPU with tests/mesh_reference.py
EXPECTED = {'scene': (1910, 3804, 4), 'random_131_5_3': (1035, 1712, 14), 'random_67_9_5': (2093, 4730, 5),
            'serpentine': (4420, 8836, 1), 'serpentine_cut': (4416, 8824, 2)}
SCENE_COMPONENT_BALL = (2, 0, 1, 3)   # the ball of component id 0 .. 3: ids follow the smallest vertex, not the balls' order
_MESH, _LABELS = {}, {}


def mesh(name):
  """(vertices, vertex_cell, faces) of a fixture grid: CPU only, computed once, never changed."""
  if name not in _MESH:
    _MESH[name] = M.surface_nets(*GRIDS[name]())
  return _MESH[name]


def labelled(name):
  """(labels, C, comp_counts, comp_bbox) of a fixture mesh by the reference."""
  if name not in _LABELS:
    v, _, f = mesh(name)
    labels, C = components(f, len(v))
    _LABELS[name] = (labels, C) + table(v, f, labels, C)
  return _LABELS[name]


def renumbered(name, order, seed):
  """The fixture with vertex `old` renamed perm[old] and its triangles shuffled: (vertices, faces).  order: 'random' or 'reversed'."""
  v, _, f = mesh(name)
  V = len(v)
  rs = np.random.RandomState(seed)
  perm = rs.permutation(V) if order == 'random' else np.arange(V)[::-1]
  nv = np.empty_like(v)
  nv[perm] = v
  nf = perm[f].astype(np.int32)
  return nv, nf[rs.permutation(len(nf))]
