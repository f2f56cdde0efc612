"""Surface nets in NumPy, float32: the definition of include/nerfies_amd.h (nrf_mesh_count / nrf_mesh_emit / nrf_mesh_snap) restated
with loops, for tiny grids.  Not a test: the mesh tests import it.  Also the invariant checkers of a triangle mesh (edge use
counts, opposite edge directions, Euler characteristic, signed volume) and the check grids.

A grid is `sigma[i, j, k]` of shape (X, Y, Z) (any strides), sample (i, j, k) at origin + idx * step."""
from fractions import Fraction

import numpy as np

F32 = np.float32
CORNERS = [(b & 1, (b >> 1) & 1, (b >> 2) & 1) for b in range(8)]   # corner bit b = di + 2 dj + 4 dk


def surface_nets(sigma, origin, step, threshold):
  """(vertices (V,3) float32, vertex_cell (V,) int32, faces (F,3) int32) of the grid, in the contract's order."""
  s = np.asarray(sigma, dtype=F32)
  X, Y, Z = s.shape
  thr = F32(threshold)
  origin = np.asarray(origin, dtype=F32)
  step = np.asarray(step, dtype=F32)
  with np.errstate(all='ignore'):
    inside = s > thr                                            # strict: NaN is outside
  cx, cy, cz = X - 1, Y - 1, Z - 1
  vmap = -np.ones((cx, cy, cz), dtype=np.int64)
  verts, cells = [], []
  for k in range(cz):
    for j in range(cy):
      for i in range(cx):
        ins = [bool(inside[i + d[0], j + d[1], k + d[2]]) for d in CORNERS]
        if all(ins) or not any(ins):
          continue
        acc = np.zeros(3, dtype=F32)
        count = 0
        for a in range(8):
          for axis in range(3):
            if (a >> axis) & 1:
              continue
            b = a | (1 << axis)
            if ins[a] == ins[b]:
              continue
            sa = s[i + CORNERS[a][0], j + CORNERS[a][1], k + CORNERS[a][2]]
            sb = s[i + CORNERS[b][0], j + CORNERS[b][1], k + CORNERS[b][2]]
            with np.errstate(all='ignore'):
              t = F32(F32(thr - sa) / F32(sb - sa))
            if not np.isfinite(t):
              t = F32(0.5)
            elif t < 0:
              t = F32(0)
            elif t > 1:
              t = F32(1)
            p = np.array(CORNERS[a], dtype=F32)
            p[axis] = F32(p[axis] + t)
            acc = (acc + p).astype(F32)
            count += 1
        local = (acc / F32(count)).astype(F32)
        idx = np.array([i, j, k], dtype=F32)
        v = ((idx + local).astype(F32) * step).astype(F32)
        v = (v + origin).astype(F32)
        vmap[i, j, k] = len(verts)
        verts.append(v)
        cells.append(i + cx * (j + cy * k))
  faces = []
  for k in range(cz):
    for j in range(cy):
      for i in range(cx):
        c = (i, j, k)
        for ax in range(3):
          u, v = (ax + 1) % 3, (ax + 2) % 3
          if c[u] < 1 or c[v] < 1:
            continue
          n = list(c)
          n[ax] += 1
          if inside[c] == inside[tuple(n)]:
            continue
          eu, ev = np.eye(3, dtype=np.int64)[u], np.eye(3, dtype=np.int64)[v]
          cc = np.array(c)
          q = [vmap[tuple(cc - eu - ev)], vmap[tuple(cc - ev)], vmap[tuple(cc)], vmap[tuple(cc - eu)]]
          assert min(q) >= 0
          if not inside[c]:
            q = q[::-1]
          faces.append((q[0], q[1], q[2]))
          faces.append((q[0], q[2], q[3]))
  return (np.array(verts, dtype=F32).reshape(-1, 3), np.array(cells, dtype=np.int32).reshape(-1),
          np.array(faces, dtype=np.int32).reshape(-1, 3))


# ---- nrf_mesh_snap on the host, every step rounded once to float32 from the exact rational ----
def _round32(t):
  """The float32 nearest to the exact rational t, ties to even; +-inf beyond the format's range."""
  big = Fraction(float(np.finfo(F32).max)) + Fraction(2) ** 103
  if t >= big:
    return F32(np.inf)
  if t <= -big:
    return F32(-np.inf)
  with np.errstate(all='ignore'):
    f = F32(float(t))
  if not np.isfinite(f):
    f = F32(np.finfo(F32).max) if t > 0 else F32(-np.finfo(F32).max)
  best = None
  for c in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
    if not np.isfinite(c):
      continue
    d = abs(Fraction(float(c)) - t)
    even = (int(np.array(c, dtype=F32).view(np.uint32)) & 1) == 0
    if best is None or d < best[0] or (d == best[0] and even):
      best = (d, c)
  return F32(best[1])


def _fr(x):
  return Fraction(float(x))


def snap(vertices, vertex_cell, sigma_at, grad_at, origin, step, dims, threshold):
  """One Newton step per vertex, then the clamp to the vertex's own cell, as the header states them."""
  v = np.array(vertices, dtype=F32).reshape(-1, 3).copy()
  g = np.asarray(grad_at, dtype=F32).reshape(-1, 3)
  sg = np.asarray(sigma_at, dtype=F32).reshape(-1)
  origin = np.asarray(origin, dtype=F32)
  step = np.asarray(step, dtype=F32)
  thr = F32(threshold)
  cx, cy = dims[0] - 1, dims[1] - 1
  for r in range(v.shape[0]):
    if not np.isfinite(g[r]).all() or not np.isfinite(sg[r]):
      continue                                                   # s or sigma not finite
    s = _round32(_fr(g[r, 0]) * _fr(g[r, 0]))
    if np.isfinite(s):
      s = _round32(_fr(g[r, 1]) * _fr(g[r, 1]) + _fr(s))
    if np.isfinite(s):
      s = _round32(_fr(g[r, 2]) * _fr(g[r, 2]) + _fr(s))
    if not np.isfinite(s) or not s > 0:
      continue
    d = _round32(_fr(sg[r]) - _fr(thr))
    q = _round32(_fr(d) / _fr(s)) if np.isfinite(d) else (F32(np.inf) if d > 0 else F32(-np.inf))
    cell = int(vertex_cell[r])
    idx = (cell % cx, (cell // cx) % cy, cell // (cx * cy))
    for c in range(3):
      if np.isfinite(q):
        x = _round32(-_fr(q) * _fr(g[r, c]) + _fr(v[r, c]))
      else:
        with np.errstate(all='ignore'):
          x = F32(np.float64(-q) * np.float64(g[r, c]) + np.float64(v[r, c]))   # inf arithmetic: +-inf, or NaN from inf * 0
      e0 = F32(origin[c] + F32(F32(idx[c]) * step[c]))
      e1 = F32(origin[c] + F32(F32(idx[c] + 1) * step[c]))
      lo, hi = min(e0, e1), max(e0, e1)
      if not x >= lo:
        x = lo                                                   # a NaN lands here too
      elif x > hi:
        x = hi
      v[r, c] = x
  return v


# ---- invariants of a triangle mesh ----
def edge_report(faces):
  """(every undirected edge is in exactly two faces, every directed edge's opposite appears exactly once, number of edges)."""
  directed = {}
  for f in np.asarray(faces).reshape(-1, 3):
    for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
      directed[(int(a), int(b))] = directed.get((int(a), int(b)), 0) + 1
  undirected = {}
  for (a, b), n in directed.items():
    key = (min(a, b), max(a, b))
    undirected[key] = undirected.get(key, 0) + n
  closed = all(n == 2 for n in undirected.values())
  opposite = all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
  return closed, opposite, len(undirected)


def euler_characteristic(num_vertices, faces):
  return int(num_vertices) - edge_report(faces)[2] + len(np.asarray(faces).reshape(-1, 3))


def signed_volume(vertices, faces):
  v = np.asarray(vertices, dtype=np.float64)
  f = np.asarray(faces).reshape(-1, 3)
  return float(np.einsum('ij,ij->i', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---- the check grids ----
CENTRE = (0.07, -0.05, 0.03)


def _positions(dims, origin, step):
  idx = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing='ij'), -1).astype(np.float64)
  return np.asarray(origin, np.float64) + idx * np.asarray(step, np.float64)


def sphere_grid():
  dims, origin, step = (13, 11, 9), (-1.0, -0.9, -0.8), (2.0 / 12, 1.8 / 10, 1.6 / 8)
  p = _positions(dims, origin, step) - np.asarray(CENTRE)
  return (0.6 - np.sqrt((p ** 2).sum(-1))).astype(F32), origin, step, 0.0


def torus_grid():
  dims, origin, step = (17, 15, 9), (-1.0, -0.9, -0.5), (2.0 / 16, 1.8 / 14, 1.0 / 8)
  p = _positions(dims, origin, step) - np.asarray(CENTRE)
  ring = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - 0.55
  return (0.22 - np.sqrt(ring ** 2 + p[..., 2] ** 2)).astype(F32), origin, step, 0.0


def centre_grid():
  s = np.zeros((3, 3, 3), dtype=F32)
  s[1, 1, 1] = 1.0
  return s, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.5


def corner_grid():
  s = np.zeros((2, 2, 2), dtype=F32)
  s[0, 0, 0] = 1.0
  return s, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.5


CHECK_GRIDS = {'sphere': sphere_grid, 'torus': torus_grid, 'centre': centre_grid, 'corner': corner_grid}
# (V, F, chi) quoted by the definition's author for these grids; chi None where there is no face
EXPECTED = {'sphere': (210, 416, 2), 'torus': (402, 804, 0), 'centre': (8, 12, 2), 'corner': (1, 0, None)}
