"""The mesh rasteriser's definition (include/nerfies_amd.h, "Mesh rasteriser") restated in NumPy: int64 edge functions on coordinates
snapped to 1/256 pixel, float32 depth and barycentrics with one rounding per operation in the header's order, ownership by the
smallest 64-bit key.  It has no notion of the kernels' 256-pixel split beyond counting the triangles whose pixel box is larger.

Also here: the cases the host test and the GPU test share (three inputs on which every pixel of the union must be owned exactly
once, and a sphere seen by a distorted camera), so that both tests speak of the same inputs."""
import numpy as np

F32 = np.float32
EDGES = ((1, 2), (2, 0), (0, 1))
LIMIT = F32(1048576.0)
SMALL_BOX = 256   # pixels of a pixel box the kernels still draw with one thread: counted in the status, never seen in the image


def usable(screen, near):
  """(V,) bool: z > near, |px| <= 2^20, |py| <= 2^20, each false for NaN."""
  s = np.asarray(screen, dtype=F32).reshape(-1, 3)
  with np.errstate(invalid='ignore'):
    return (s[:, 2] > F32(near)) & (np.abs(s[:, 0]) <= LIMIT) & (np.abs(s[:, 1]) <= LIMIT)


def snap(screen, ok):
  """(V, 2) int64 sub-pixel coordinates; rows that are not usable hold 0."""
  s = np.asarray(screen, dtype=F32).reshape(-1, 3)
  out = np.zeros((len(s), 2), np.int64)
  out[ok] = np.rint(s[ok, :2] * F32(256.0)).astype(np.int64)
  return out


def triangles(screen, faces, W, H, near=0.0):
  """Yields (t, X (3,), Y (3,), z (3,) float32, s, sA, i0, i1, j0, j1) for every triangle that passes the skip rules."""
  s = np.asarray(screen, dtype=F32).reshape(-1, 3)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  V = len(s)
  ok = usable(s, near)
  xy = snap(s, ok)
  for t, tri in enumerate(f):
    if (tri < 0).any() or (tri >= V).any() or not ok[tri].all():
      continue
    X, Y = [int(v) for v in xy[tri, 0]], [int(v) for v in xy[tri, 1]]
    A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if A == 0:
      continue
    sg = 1 if A > 0 else -1
    i0, i1 = max(0, -((128 - min(X)) // 256)), min(W - 1, (max(X) - 128) // 256)   # -(-a // b) is the ceiling
    j0, j1 = max(0, -((128 - min(Y)) // 256)), min(H - 1, (max(Y) - 128) // 256)
    if i0 > i1 or j0 > j1:
      continue
    yield t, X, Y, s[tri, 2].copy(), sg, sg * A, i0, i1, j0, j1


def shade(X, Y, z, sg, sA, i0, i1, j0, j1):
  """Over the pixel box: (covered (h, w) bool, depth (h, w) float32, bary (h, w, 3) float32)."""
  Px = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[None, :]
  Py = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[:, None]
  covered = np.ones((j1 - j0 + 1, i1 - i0 + 1), bool)
  q = []
  area = F32(np.int64(sA))
  with np.errstate(all='ignore'):
    for k, (a, b) in enumerate(EDGES):
      dx, dy = sg * (X[b] - X[a]), sg * (Y[b] - Y[a])
      E = dx * (Py - Y[a]) - dy * (Px - X[a])
      top_left = dy < 0 or (dy == 0 and dx > 0)
      covered &= (E > 0) | ((E == 0) & top_left)
      l = E.astype(F32) / area
      q.append(l / F32(z[k]))
    w = (q[0] + q[1]) + q[2]
    depth = F32(1.0) / w
    bary = np.stack([q[0] / w, q[1] / w, q[2] / w], -1)
  return covered, depth.astype(F32), bary.astype(F32)


def _walk(screen, faces, W, H, near):
  """Yields (t, rows, cols, depth bits (n,) uint32, bary (n, 3), large) over the covered pixels of every drawn triangle."""
  for t, X, Y, z, sg, sA, i0, i1, j0, j1 in triangles(screen, faces, W, H, near):
    covered, depth, bary = shade(X, Y, z, sg, sA, i0, i1, j0, j1)
    jj, ii = np.nonzero(covered)
    yield t, jj + j0, ii + i0, depth[jj, ii].view(np.uint32), bary[jj, ii], (i1 - i0 + 1) * (j1 - j0 + 1) > SMALL_BOX


def draw(screen, faces, W, H, near=0.0):
  """(face_id (H, W) int32, depth (H, W) float32, bary (H, W, 3) float32, status [drawn, large, covered, 0])."""
  keys = np.full((H, W), np.uint64(0xffffffffffffffff), np.uint64)
  bary = np.zeros((H, W, 3), F32)
  drawn = large = 0
  for t, jj, ii, bits, b, big in _walk(screen, faces, W, H, near):
    drawn += 1
    large += int(big)
    key = (bits.astype(np.uint64) << np.uint64(32)) | np.uint64(t)
    win = key < keys[jj, ii]
    keys[jj[win], ii[win]] = key[win]
    bary[jj[win], ii[win]] = b[win]
  empty = keys == np.uint64(0xffffffffffffffff)
  face_id = np.where(empty, -1, (keys & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)
  depth = np.where(empty, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(F32)
  bary[empty] = 0
  return face_id, depth, bary, [drawn, large, int((~empty).sum()), 0]


def coverage_count(screen, faces, W, H, near=0.0):
  """(H, W) int: how many triangles cover each pixel."""
  count = np.zeros((H, W), np.int64)
  for _, jj, ii, _, _, _ in _walk(screen, faces, W, H, near):
    np.add.at(count, (jj, ii), 1)
  return count


def tie_pixels(screen, faces, W, H, near=0.0):
  """(H, W) bool: the pixels whose two smallest candidate depths have equal bits but different faces.  There the owner is decided by
  the face index, so a permutation of the faces may hand the pixel to another face (with the same depth bits)."""
  best = np.full((H, W), np.uint64(1) << np.uint64(40), np.uint64)
  ties = np.zeros((H, W), np.int64)
  for _, jj, ii, bits, _, _ in _walk(screen, faces, W, H, near):
    bits = bits.astype(np.uint64)
    cur = best[jj, ii]
    lower, same = bits < cur, bits == cur
    best[jj[lower], ii[lower]] = bits[lower]
    ties[jj[lower], ii[lower]] = 1
    ties[jj[same], ii[same]] += 1
  return ties >= 2


def interpolate(face_id, bary, faces, attributes, background=None):
  """(P, A) float32: (b0 * a0 + b1 * a1) + b2 * a2 in float32; the background row where face_id < 0."""
  fid = np.asarray(face_id).reshape(-1)
  b = np.asarray(bary, dtype=F32).reshape(-1, 3)
  a = np.asarray(attributes, dtype=F32)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  bg = np.zeros(a.shape[1], F32) if background is None else np.asarray(background, dtype=F32)
  out = np.broadcast_to(bg, (len(fid), a.shape[1])).copy()
  hit = (fid >= 0) & (fid < len(f))
  if hit.any():
    tri = f[fid[hit]]
    inside = ((tri >= 0) & (tri < len(a))).all(1)
    rows = np.nonzero(hit)[0][inside]
    tri = tri[inside]
    with np.errstate(all='ignore'):
      out[rows] = (b[rows, 0:1] * a[tri[:, 0]] + b[rows, 1:2] * a[tri[:, 1]]) + b[rows, 2:3] * a[tri[:, 2]]
  return out


def visibility(face_id, faces, V):
  fid = np.asarray(face_id).reshape(-1)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  vis = np.zeros(V, np.uint8)
  corners = f[np.unique(fid[(fid >= 0) & (fid < len(f))])].reshape(-1)
  vis[corners[(corners >= 0) & (corners < V)]] = 1
  return vis


# ---- the shared cases ----

def _screen(points_sub, z):
  """Sub-pixel integer coordinates -> a float32 screen array (exact: |X| < 2^24)."""
  p = np.asarray(points_sub, dtype=np.float64)
  return np.concatenate([p / 256.0, np.asarray(z, np.float64).reshape(-1, 1)], 1).astype(F32)


def fan_case():
  """Eight triangles around a vertex on a pixel centre, rim vertices on pixel centres, each with a random orientation and a random
  first corner; 12 x 10 image.  -> (screen, faces, W, H, polygon (rim, sub-pixel units))."""
  rng = np.random.RandomState(0)
  W, H = 12, 10
  centre = (256 * 6 + 128, 256 * 5 + 128)
  rim = [(256 * i + 128, 256 * j + 128) for i, j in [(1, 1), (6, 0), (11, 1), (11, 5), (10, 9), (6, 9), (1, 8), (0, 5)]]
  faces = []
  for k in range(8):
    tri = [0, 1 + k, 1 + (k + 1) % 8]
    if rng.rand() < 0.5:
      tri = [tri[0], tri[2], tri[1]]
    r = rng.randint(3)
    faces.append(tri[r:] + tri[:r])
  z = 1.0 + 0.25 * np.arange(9)
  return _screen([centre] + rim, z), np.array(faces, np.int32), W, H, rim


def quad_cases():
  """Both splits of a quad over the whole 12 x 10 image, corners on pixel corners, in both orientations."""
  W, H = 12, 10
  q = [(0, 0), (256 * W, 0), (256 * W, 256 * H), (0, 256 * H)]
  screen = _screen(q, [1.0, 2.0, 3.0, 1.5])
  return [(screen, np.array(f, np.int32), W, H, q) for f in ([[0, 1, 2], [0, 2, 3]], [[1, 0, 3], [3, 2, 1]])]


def centre_quad_case():
  """A quad whose edges run through pixel centres (corners on the centres of (2,2), (9,2), (9,7), (2,7)); 12 x 10 image."""
  W, H = 12, 10
  q = [(256 * 2 + 128, 256 * 2 + 128), (256 * 9 + 128, 256 * 2 + 128), (256 * 9 + 128, 256 * 7 + 128), (256 * 2 + 128, 256 * 7 + 128)]
  return _screen(q, [2.0, 1.0, 1.0, 2.0]), np.array([[0, 1, 2], [0, 2, 3]], np.int32), W, H, q


def exactly_once_cases():
  out = {'fan': fan_case(), 'centre_quad': centre_quad_case()}
  for n, c in enumerate(quad_cases()):
    out[f'quad_split{n}'] = c
  return out


def polygon_sides(polygon, W, H):
  """Of a convex polygon in sub-pixel units, per pixel centre: (strictly inside (H, W) bool, on the boundary (H, W) bool), exactly."""
  P = np.asarray(polygon, dtype=np.int64)
  area2 = sum(int(P[k][0]) * int(P[(k + 1) % len(P)][1]) - int(P[(k + 1) % len(P)][0]) * int(P[k][1]) for k in range(len(P)))
  sg = 1 if area2 > 0 else -1
  Px = (256 * np.arange(W, dtype=np.int64) + 128)[None, :]
  Py = (256 * np.arange(H, dtype=np.int64) + 128)[:, None]
  inside = np.ones((H, W), bool)
  closed = np.ones((H, W), bool)
  for k in range(len(P)):
    a, b = P[k], P[(k + 1) % len(P)]
    E = sg * ((b[0] - a[0]) * (Py - a[1]) - (b[1] - a[1]) * (Px - a[0]))
    inside &= E > 0
    closed &= E >= 0
  return inside, closed & ~inside


# The sphere of the GPU test: density r0 - |x| on a 16^3 grid of the unit box, level set at 0.
SPHERE_R0 = 0.35
SPHERE_DIMS = (16, 16, 16)
SPHERE_ORIGIN = (-0.5, -0.5, -0.5)
SPHERE_STEP = (1.0 / 15,) * 3
SPHERE_IMAGE = (64, 48)


def sphere_sigma():
  idx = np.stack(np.meshgrid(*[np.arange(n) for n in SPHERE_DIMS], indexing='ij'), -1).astype(np.float64)
  p = np.asarray(SPHERE_ORIGIN) + idx * np.asarray(SPHERE_STEP)
  return (SPHERE_R0 - np.sqrt((p ** 2).sum(-1))).astype(F32)


def sphere_camera():
  """camera_oracle.make_camera arguments of a distorted camera at about 1.6 from the centre, the sphere filling most of 64 x 48."""
  position = np.array([0.55, -0.35, -1.45])
  axis = -position / np.linalg.norm(position)
  right = np.cross(axis, [0.0, 1.0, 0.0])
  right /= np.linalg.norm(right)
  orientation = np.stack([right, np.cross(axis, right), axis])
  return dict(orientation=orientation, position=position, focal_length=92.0, principal_point=(31.3, 24.6), image_size=SPHERE_IMAGE,
              skew=0.05, pixel_aspect_ratio=1.02, radial_distortion=(0.08, -0.03, 0.01), tangential_distortion=(0.004, -0.003))
