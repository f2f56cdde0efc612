"""Mesh clean-up on the GPU (nrf_mesh_components / nrf_mesh_component_table / nrf_mesh_submesh_* / nrf_mesh_gather_rows,
evaluation.mesh_components / submesh / clean_mesh / extract_mesh(clean=), export_density --mesh_keep).

The entries against tests/mesh_components_reference.py (the header's definitions restated in NumPy), exactly: labels, tables, maps and
faces as integers, gathered rows and boxes as bits.  There is no tolerance anywhere; where a field is involved its own queries are
compared with themselves, bit for bit (a query's row does not depend on the launch it ran in)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import helpers as H
import mesh_components_reference as R
import mesh_reference as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
CANARY_I, CANARY_F = -77777, -12345.5


def _hand():
  """Invalid triangles (an index of -1, an index of V), a triangle (a, a, b), NaN and -0.0 coordinates, an all-NaN component."""
  v = np.array([[0, 1, 2], [np.nan, -0.0, 5], [3, 0.0, np.nan], [np.nan, np.nan, np.nan], [7, 7, 7]], dtype=np.float32)
  f = np.array([[0, 1, 2], [2, 2, 1], [0, 1, 5], [-1, 0, 1], [4, 4, 4]], dtype=np.int32)
  return v, f


def _junk():
  rs = np.random.RandomState(11)
  v = rs.randn(300, 3).astype(np.float32)
  v[rs.randint(0, 300, 40), rs.randint(0, 3, 40)] = np.nan
  v[rs.randint(0, 300, 40), rs.randint(0, 3, 40)] = -0.0
  return v, rs.randint(-20, 320, (260, 3)).astype(np.int32)     # most triangles valid, many invalid, some degenerate


MESHES = {name: (lambda name=name: (R.mesh(name)[0], R.mesh(name)[2])) for name in R.EXPECTED}
MESHES.update({
    'serpentine_shuffled': lambda: R.renumbered('serpentine', 'random', 5),
    'serpentine_reversed': lambda: R.renumbered('serpentine', 'reversed', 6),
    'serpentine_cut_shuffled': lambda: R.renumbered('serpentine_cut', 'random', 7),
    'serpentine_cut_reversed': lambda: R.renumbered('serpentine_cut', 'reversed', 8),
    'no_vertices': lambda: (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
    'no_triangles': lambda: (np.arange(15, dtype=np.float32).reshape(5, 3), np.zeros((0, 3), np.int32)),
    'hand': _hand,
    'junk': _junk,
})
_REF = {}


def reference(name):
  """(vertices, faces, labels, C, comp_counts, comp_bbox) of a case: CPU only, computed once, never changed."""
  if name not in _REF:
    v, f = MESHES[name]()
    labels, nc = R.components(f, len(v))
    _REF[name] = (v, f, labels, nc) + R.table(v, f, labels, nc)
  return _REF[name]


def _masks(name):
  """The keep masks a case's submesh is checked with: every component alone (up to five), a seeded random half, all, none."""
  v, f, labels, nc = reference(name)[:4]
  rs = np.random.RandomState(3)
  masks = [labels == c for c in range(min(nc, 5))]
  masks += [rs.rand(len(v)) < 0.5, np.ones(len(v), bool), np.zeros(len(v), bool)]
  return [m.astype(np.uint8) * np.uint8(1 + 6 * (i % 2)) for i, m in enumerate(masks)]   # any nonzero byte keeps


def _bits(t):
  return t.contiguous().view(torch.int32)


def _dev(a):
  return torch.from_numpy(np.array(a)).to(H.DEV)   # a copy: the references are read-only


class _Raw:
  """The entries themselves on device tensors, with PAD canary elements behind every output."""

  def __init__(self, vertices, faces):
    from nerfies_amd import lib as L
    self.L, self.lib = L, L.load_library()
    self.V, self.F = len(vertices), len(faces)
    self.vertices, self.faces = _dev(vertices), _dev(faces)
    self.stream = torch.cuda.current_stream(torch.device(H.DEV)).cuda_stream
    self.cws = self._ws(self.lib.nrf_mesh_components_workspace_bytes)
    self.sws = self._ws(self.lib.nrf_mesh_submesh_workspace_bytes)

  def _ws(self, sizer):
    n = C.c_size_t(0)
    self.L.check(sizer(self.V, self.F, C.byref(n)), self.lib)
    return torch.full(((n.value + 3) // 4,), CANARY_I, dtype=torch.int32, device=H.DEV)

  def components(self):
    labels = torch.full((self.V + PAD,), CANARY_I, dtype=torch.int32, device=H.DEV)
    counts = torch.full((1 + PAD,), CANARY_I, dtype=torch.int32, device=H.DEV)
    self.L.check(self.lib.nrf_mesh_components(self.faces.data_ptr(), self.F, self.V, labels.data_ptr(), counts.data_ptr(),
                                              self.cws.data_ptr(), self.cws.numel() * 4, self.stream), self.lib)
    assert bool((labels[self.V:] == CANARY_I).all()) and bool((counts[1:] == CANARY_I).all())
    self.labels = labels
    return labels[:self.V], int(counts[0]), tuple(self.cws[:4].tolist())

  def table(self, rows, max_components, boxes=True):
    cc = torch.full((rows + PAD, 2), CANARY_I, dtype=torch.int32, device=H.DEV)
    bb = torch.full((rows + PAD, 6), CANARY_F, dtype=torch.float32, device=H.DEV)
    self.L.check(self.lib.nrf_mesh_component_table(self.faces.data_ptr(), self.F, self.vertices.data_ptr() if boxes else None, self.V,
                                                   self.labels.data_ptr(), max_components, cc.data_ptr(), bb.data_ptr() if boxes else None,
                                                   self.cws.data_ptr(), self.cws.numel() * 4, self.stream), self.lib)
    return cc, bb, tuple(self.cws[:4].tolist())

  def count(self, keep):
    self.keep = _dev(keep)
    counts = torch.full((2 + PAD,), CANARY_I, dtype=torch.int32, device=H.DEV)
    self.L.check(self.lib.nrf_mesh_submesh_count(self.keep.data_ptr(), self.V, self.faces.data_ptr(), self.F, counts.data_ptr(),
                                                 self.sws.data_ptr(), self.sws.numel() * 4, self.stream), self.lib)
    assert bool((counts[2:] == CANARY_I).all())
    return tuple(counts[:2].tolist())

  def emit(self, rows_t, max_v, max_t):
    vmap = torch.full((self.V + PAD,), CANARY_I, dtype=torch.int32, device=H.DEV)
    tris = torch.full((rows_t + PAD, 3), CANARY_I, dtype=torch.int32, device=H.DEV)
    self.L.check(self.lib.nrf_mesh_submesh_emit(self.keep.data_ptr(), self.V, self.faces.data_ptr(), self.F, max_v, max_t, vmap.data_ptr(),
                                                tris.data_ptr(), self.sws.data_ptr(), self.sws.numel() * 4, self.stream), self.lib)
    return vmap, tris, tuple(self.sws[:4].tolist())

  def gather(self, src, vmap, rows, max_rows):
    dst = torch.full((rows + PAD,) + tuple(src.shape[1:]), CANARY_I, dtype=torch.int32, device=H.DEV).view(src.dtype)
    width = src[0].numel() * src.element_size() // 4
    self.L.check(self.lib.nrf_mesh_gather_rows(src.data_ptr(), width, vmap.data_ptr(), src.shape[0], dst.data_ptr(), max_rows, self.stream),
                 self.lib)
    return dst


def _intact(t):
  return bool((_bits(t) == CANARY_I).all()) if t.dtype == torch.int32 else bool((t == CANARY_F).all())


@pytest.mark.parametrize('name', sorted(MESHES))
def test_entries_match_the_reference(name):
  v, f, labels, nc, counts, box = reference(name)
  V, F = len(v), len(f)
  if name in R.EXPECTED:
    assert (V, F, nc) == R.EXPECTED[name]
  raw = _Raw(v, f)
  got, gc, status = raw.components()
  assert gc == nc and status[0] == nc and status[2] == 0, (name, gc, nc, status)       # the loop-cap error word stays 0
  assert torch.equal(got.cpu(), torch.from_numpy(labels)), name
  cc, bb, status = raw.table(nc, nc)
  assert status[:3] == (nc, nc, 0)
  assert torch.equal(cc[:nc].cpu(), torch.from_numpy(counts)), name
  assert torch.equal(_bits(bb[:nc].cpu()), _bits(torch.from_numpy(box))), name
  assert _intact(cc[nc:]) and _intact(bb[nc:])
  cc2, bb2, _ = raw.table(nc, nc + 7, boxes=False)                                      # without vertices: the counts alone
  assert torch.equal(cc2[:nc], cc[:nc]) and _intact(cc2[nc:]) and _intact(bb2)
  for keep in _masks(name):
    vmap, faces = R.submesh(keep, f, V)
    nv, nt = int((vmap >= 0).sum()), len(faces)
    assert raw.count(keep) == (nv, nt), name
    gm, gt, status = raw.emit(nt, nv, nt)
    assert status == (nv, nt, nv, nt)
    assert torch.equal(gm[:V].cpu(), torch.from_numpy(vmap)) and torch.equal(gt[:nt].cpu(), torch.from_numpy(faces)), name
    assert _intact(gm[V:]) and _intact(gt[nt:])
    if V:
      rows = raw.gather(raw.vertices, gm, nv, nv)
      assert torch.equal(_bits(rows[:nv].cpu()), _bits(torch.from_numpy(R.gather_rows(v, vmap)))) and _intact(_bits(rows[nv:]))


# The ranking rule by itself (no triangle: a slot is the cumsum of the mask): one lane, the sides of a wave (64), of a round (256), of a
# workgroup (1024), several workgroups, and 1026 workgroup totals: the one-workgroup scan's threads then own runs of 2, the last cut.
RULE_V = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 1024 * 1024 + 1025)
NO_FACES = np.zeros((0, 3), np.int32)


def _rule_mask(kind, V):
  if kind == 'random':
    return (np.random.RandomState(V % 9973).rand(V) < 0.5).astype(np.uint8)
  return {'all': np.ones(V, np.uint8), 'none': np.zeros(V, np.uint8), 'alternate': (np.arange(V) % 2 == 0).astype(np.uint8)}[kind]


@pytest.mark.parametrize('kind', ['all', 'none', 'alternate', 'random'])
@pytest.mark.parametrize('V', RULE_V)
def test_the_ranking_rule_alone(V, kind):
  keep = _rule_mask(kind, V)
  vmap, faces = R.submesh(keep, NO_FACES, V)
  nv = int(keep.sum())
  assert len(faces) == 0 and int((vmap >= 0).sum()) == nv and (nv == 0 or vmap.max() == nv - 1)
  raw = _Raw(np.zeros((V, 0), np.float32), NO_FACES)
  assert raw.count(keep) == (nv, 0), (V, kind)
  gm, gt, status = raw.emit(0, nv, 0)
  assert status == (nv, 0, nv, 0), (V, kind, status)
  assert torch.equal(gm[:V].cpu(), torch.from_numpy(vmap)), (V, kind)
  assert _intact(gm[V:]) and _intact(gt)


def test_components_without_triangles_across_1026_workgroups():
  V = RULE_V[-1]
  got, gc, status = _Raw(np.zeros((V, 0), np.float32), NO_FACES).components()
  assert gc == V and status[0] == V and status[2] == 0
  assert torch.equal(got, torch.arange(V, dtype=torch.int32, device=H.DEV))                 # every vertex is its own component's root


def test_scene_components_are_the_balls_alone():
  from nerfies_amd import evaluation
  v, cells, f = R.mesh('scene')
  mesh = {'vertices': _dev(v), 'vertex_cell': _dev(cells), 'faces': _dev(f)}
  comps = evaluation.mesh_components(mesh['vertices'], mesh['faces'])
  assert comps['num_vertices'].tolist() == [28, 1346, 520, 16] and comps['num_triangles'].tolist() == [52, 2688, 1036, 28]
  labels = comps['labels']
  assert [int((labels == c).nonzero()[0]) for c in range(4)] == [0, 28, 521, 1894]
  box = R.labelled('scene')[3]
  assert torch.equal(_bits(torch.cat([comps['bbox_min'], comps['bbox_max']], 1).cpu()), _bits(torch.from_numpy(box)))
  for cid, ball in enumerate(R.SCENE_COMPONENT_BALL):
    sub = evaluation.submesh(mesh, labels == cid)
    bv, bc, bf = R.mesh(f'ball{ball}')
    assert torch.equal(_bits(sub['vertices'].cpu()), _bits(torch.from_numpy(bv))), cid
    assert torch.equal(sub['vertex_cell'].cpu(), torch.from_numpy(bc)) and torch.equal(sub['faces'].cpu(), torch.from_numpy(bf)), cid
    closed, opposite, _ = M.edge_report(sub['faces'].cpu().numpy())
    assert closed and opposite and M.euler_characteristic(len(bv), sub['faces'].cpu().numpy()) == 2
    assert torch.equal(sub['vertex_map'].cpu(), torch.from_numpy(R.submesh((labels == cid).cpu().numpy(), f, len(v))[0]))
  largest = evaluation.clean_mesh(mesh)                                                  # keep='largest': the 8.4 ball
  assert torch.equal(_bits(largest['vertices'].cpu()), _bits(torch.from_numpy(R.mesh('ball0')[0])))
  assert torch.equal(largest['faces'].cpu(), torch.from_numpy(R.mesh('ball0')[2])) and largest['components']['kept'] == [1]
  two = evaluation.clean_mesh(mesh, keep=2)                                              # the two large balls
  want = np.isin(R.labelled('scene')[0], (1, 2))
  assert two['components']['kept'] == [1, 2]
  assert torch.equal(_bits(two['vertices'].cpu()), _bits(torch.from_numpy(v[want]))) and two['faces'].shape[0] == 2688 + 1036
  assert torch.equal(two['faces'].cpu(), torch.from_numpy(R.submesh(want, f, len(v))[1]))
  everything = evaluation.clean_mesh(mesh, keep='all', min_triangles=0)
  assert torch.equal(everything['faces'], mesh['faces']) and torch.equal(_bits(everything['vertices']), _bits(mesh['vertices']))
  assert evaluation.clean_mesh(mesh, keep='all', min_triangles=53)['components']['kept'] == [1, 2]


def test_python_entries_on_degenerate_meshes():
  from nerfies_amd import evaluation
  empty = {'vertices': torch.zeros(0, 3, device=H.DEV), 'faces': torch.zeros(0, 3, dtype=torch.int32, device=H.DEV)}
  comps = evaluation.mesh_components(empty['vertices'], empty['faces'])
  assert {k: tuple(t.shape) for k, t in comps.items()} == {'labels': (0,), 'num_vertices': (0,), 'num_triangles': (0,), 'bbox_min': (0, 3),
                                                           'bbox_max': (0, 3)}
  sub = evaluation.clean_mesh(empty)
  assert tuple(sub['vertices'].shape) == (0, 3) and tuple(sub['faces'].shape) == (0, 3) and tuple(sub['vertex_map'].shape) == (0,)
  v, f = _hand()
  comps = evaluation.mesh_components(None, _dev(f), num_vertices=5)                      # no vertices: no boxes
  assert set(comps) == {'labels', 'num_vertices', 'num_triangles'} and comps['labels'].tolist() == [0, 0, 0, 1, 2]
  assert comps['num_triangles'].tolist() == [2, 0, 1]
  # submesh gathers whatever has V rows, and a (K, V, ...) tensor along its second dimension; the rest is passed on
  rs = np.random.RandomState(4)
  extra = {'vertices': _dev(v), 'faces': _dev(f), 'sigma': _dev(rs.randn(5).astype(np.float32)), 'wide': _dev(rs.randn(5, 5).astype(np.float32)),
           'ids': _dev(np.arange(5, dtype=np.int64)), 'frames': _dev(rs.randn(2, 5, 3).astype(np.float32)), 'other': _dev(rs.randn(4).astype(np.float32)),
           'note': 'kept'}
  keep = torch.tensor([True, False, True, True, True], device=H.DEV)
  sub = evaluation.submesh(extra, keep)
  idx = keep.nonzero()[:, 0]
  for k in ('vertices', 'sigma', 'wide', 'ids'):
    assert torch.equal(sub[k].view(torch.int32), extra[k][idx].contiguous().view(torch.int32)), k
  assert torch.equal(_bits(sub['frames']), _bits(extra['frames'][:, idx])) and sub['other'] is extra['other'] and sub['note'] == 'kept'
  assert sub['faces'].tolist() == [[3, 3, 3]] and sub['vertex_map'].tolist() == [0, -1, 1, 2, 3]
  with pytest.raises(ValueError, match='4-byte'):
    evaluation.submesh({'faces': _dev(f), 'rgb8': torch.zeros(5, 3, dtype=torch.uint8, device=H.DEV)}, keep)


def test_two_runs_agree_bit_for_bit():
  for name in ('serpentine_cut_shuffled', 'random_67_9_5', 'junk'):
    v, f, labels, nc = reference(name)[:4]
    keep = _masks(name)[0]
    runs = []
    for _ in range(2):
      raw = _Raw(v, f)
      got, gc, status = raw.components()
      cc, bb, _ = raw.table(nc, nc)
      nv, nt = raw.count(keep)
      gm, gt, _ = raw.emit(nt, nv, nt)
      assert status[2] == 0
      runs.append((raw.labels, cc, bb, gm, gt))
    for a, b in zip(*runs):
      assert torch.equal(_bits(a), _bits(b)), name


def test_a_short_capacity_writes_nothing_and_is_reported():
  name = 'random_131_5_3'
  v, f, labels, nc, counts, box = reference(name)
  raw = _Raw(v, f)
  assert raw.components()[1] == nc == 14
  for short in (nc - 1, 1, 0):
    cc, bb, status = raw.table(nc, short)
    assert status[:3] == (nc, 0, 0), (short, status)
    assert _intact(cc) and _intact(bb), short
  cc, bb, status = raw.table(nc, nc)
  assert status[:3] == (nc, nc, 0) and torch.equal(cc[:nc].cpu(), torch.from_numpy(counts)) and _intact(cc[nc:]) and _intact(bb[nc:])
  keep = _masks(name)[1]                                                                 # the one large component
  vmap, faces = R.submesh(keep, f, len(v))
  nv, nt = int((vmap >= 0).sum()), len(faces)
  assert raw.count(keep) == (nv, nt) and nv > 1 and nt > 1
  for max_v, max_t in ((nv - 1, nt), (nv, nt - 1), (0, 0)):
    gm, gt, status = raw.emit(nt, max_v, max_t)
    assert status == (nv, nt, 0, 0), (max_v, max_t, status)
    assert _intact(gm) and _intact(gt), (max_v, max_t)
  gm, gt, status = raw.emit(nt, nv + 10, nt + 10)                                        # larger capacities than needed change nothing
  assert status == (nv, nt, nv, nt) and torch.equal(gm[:len(v)].cpu(), torch.from_numpy(vmap)) and torch.equal(gt[:nt].cpu(), torch.from_numpy(faces))
  assert _intact(gm[len(v):]) and _intact(gt[nt:])


@pytest.mark.parametrize('width', [1, 3, 5])
def test_gather_rows(width):
  V = 2500                                                                               # ten workgroups at width 1, odd tails at 3 and 5
  rs = np.random.RandomState(width)
  keep = rs.rand(V) < 0.6
  vmap = R.submesh(keep, np.zeros((0, 3), np.int32), V)[0]
  nv = int(keep.sum())
  raw = _Raw(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
  for dtype in (np.float32, np.int32):
    src = rs.randn(V, width).astype(np.float32).view(dtype) if dtype is np.int32 else rs.randn(V, width).astype(np.float32)
    src[5, 0] = np.float32(np.nan).view(dtype) if dtype is np.int32 else np.nan          # byte for byte, whatever the bits say
    dst = raw.gather(_dev(src), _dev(vmap), nv, nv)
    assert torch.equal(_bits(dst[:nv].cpu()), _bits(torch.from_numpy(src[keep]))) and _intact(_bits(dst[nv:]))
    half = nv // 2                                                                       # rows at or past max_rows are not written
    dst = raw.gather(_dev(src), _dev(vmap), nv, half)
    assert torch.equal(_bits(dst[:half].cpu()), _bits(torch.from_numpy(src[keep][:half]))) and _intact(_bits(dst[half:]))


@pytest.mark.parametrize('name,warp_id', [('b_no_condition', None), ('g_se3', 2)])
def test_extract_mesh_cleaned_with_a_field(name, warp_id):
  from nerfies_amd import evaluation
  from test_gpu_field_gradient import ALPHA, _model
  from test_gpu_mesh import HI, LO, RES
  model, fp = _model(name)
  kw = dict(level='fine', warp_id=warp_id, warp_extra={'alpha': ALPHA})
  grid = evaluation.density_grid(model, fp, LO, HI, RES, **kw)
  thr = float(grid.reshape(-1).sort().values[grid.numel() // 2])
  step = [(h - l) / r for l, h, r in zip(LO, HI, RES)]
  origin = [l + 0.5 * s for l, s in zip(LO, step)]
  plain = evaluation.extract_mesh(model, fp, LO, HI, RES, thr, refine_steps=2, **kw)
  assert set(plain) == {'vertices', 'faces', 'normals', 'sigma', 'rgb'}                  # clean=None: the keys and bits of today
  rv, rc, rf = M.surface_nets(grid.cpu().numpy(), origin, step, thr)
  assert torch.equal(plain['faces'].cpu(), torch.from_numpy(rf)) and len(rv) == plain['vertices'].shape[0] > 50
  again = evaluation.extract_mesh(model, fp, LO, HI, RES, thr, refine_steps=2, clean=None, **kw)
  for k in plain:
    assert torch.equal(_bits(again[k]), _bits(plain[k])), k

  labels, nc = R.components(rf, len(rv))
  counts = R.table(None, rf, labels, nc)[0]
  print(f'[mesh components] {name}: V {len(rv)} F {len(rf)} C {nc}, triangles per component {sorted(counts[:, 1].tolist(), reverse=True)[:8]}')
  cleaned = evaluation.extract_mesh(model, fp, LO, HI, RES, thr, refine_steps=2, clean=dict(keep='all', min_triangles=1), **kw)
  assert set(cleaned) == set(plain) | {'vertex_map', 'components'}
  assert torch.equal(cleaned['components']['labels'].cpu(), torch.from_numpy(labels))
  mask = torch.from_numpy((counts[:, 1] >= 1)[labels]).to(H.DEV)
  want = evaluation.submesh(plain, mask)
  for k in ('vertices', 'faces', 'normals', 'sigma'):
    assert torch.equal(_bits(cleaned[k]), _bits(want[k])), k
  assert torch.equal(cleaned['vertex_map'], want['vertex_map'])

  # an explicit mask that always drops something: the vertices below the box's mid-plane in x, of the unrefined mesh
  raw = evaluation.extract_mesh_from_grid(grid, origin, step, thr, lib=model.lib)
  below = raw['vertices'][:, 0] < 0.5 * (LO[0] + HI[0])
  assert 0 < int(below.sum()) < len(rv)
  half = evaluation.submesh(raw, below)
  vertices, vertex_cell = half['vertices'], half['vertex_cell']
  md = {} if warp_id is None else {'warp': torch.tensor([[warp_id]], dtype=torch.int32, device=H.DEV)}
  q = dict(metadata=md, warp_extra={'alpha': ALPHA}, level='fine', use_warp=warp_id is not None)
  from nerfies_amd import lib as L
  g = L.grid(origin, step, grid.shape)
  for _ in range(2):                                                                     # extract_mesh's refinement on the kept rows alone
    got = model.query_gradient(fp, vertices, outputs=('sigma', 'grad_sigma'), **q)
    L.check(model.lib.nrf_mesh_snap(vertices.data_ptr(), vertex_cell.data_ptr(), got['sigma'].data_ptr(), got['grad_sigma'].data_ptr(),
                                    C.byref(g), thr, vertices.shape[0], torch.cuda.current_stream(torch.device(H.DEV)).cuda_stream), model.lib)
  got = model.query_gradient(fp, vertices, outputs=('sigma', 'normals'), **q)
  want = evaluation.submesh(plain, below)
  assert want['vertices'].shape[0] == int(below.sum()) < len(rv)
  assert torch.equal(_bits(vertices), _bits(want['vertices'])) and torch.equal(half['faces'], want['faces'])
  assert torch.equal(_bits(got['normals']), _bits(want['normals'])) and torch.equal(_bits(got['sigma']), _bits(want['sigma']))


def test_export_density_with_a_cleaned_mesh_end_to_end(tmp_path):
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
  common = args + ['--canonical', '--resolution', '8']
  gin.clear_config()
  plain = export_density.main(common + ['--threshold', '1e30'])
  assert set(plain) == {'npy', 'ply', 'resolution', 'num_vertices', 'bbox'}             # no key is added to a run without --mesh
  grid = np.load(plain['npy'])
  thr = repr(float(np.sort(grid.ravel())[grid.size // 2]))
  gin.clear_config()
  before = export_density.main(common + ['--threshold', thr, '--mesh', '--mesh_refine', '1'])
  blob_before = open(before['mesh_ply'], 'rb').read()
  gin.clear_config()
  same = export_density.main(common + ['--threshold', thr, '--mesh', '--mesh_refine', '1', '--mesh_keep', 'all'])
  assert open(same['mesh_ply'], 'rb').read() == blob_before                             # --mesh_keep all: the byte-identical file
  assert same['num_mesh_components'] == before['num_mesh_components'] >= 1
  gin.clear_config()
  res = export_density.main(common + ['--threshold', thr, '--mesh', '--mesh_refine', '1', '--mesh_keep', 'largest'])
  V, F = res['num_mesh_vertices'], res['num_mesh_faces']
  assert 0 < V <= before['num_mesh_vertices'] and 0 < F <= before['num_mesh_faces']
  assert res['num_mesh_components'] == before['num_mesh_components']
  blob = open(res['mesh_ply'], 'rb').read()
  end = blob.index(b'end_header\n') + len(b'end_header\n')
  head = blob[:end].decode('ascii').splitlines()
  assert f'element vertex {V}' in head and f'element face {F}' in head
  assert len(blob) == end + V * (6 * 4 + 3) + F * (1 + 3 * 4)
  face = np.frombuffer(blob, dtype=[('n', 'u1'), ('idx', '<i4', 3)], count=F, offset=end + V * 27)
  assert (face['n'] == 3).all() and face['idx'].min() >= 0 and face['idx'].max() < V
  assert R.components(face['idx'], V)[1] == 1                                            # what was written is one component
  print(f'[export --mesh_keep largest] C {res["num_mesh_components"]}: V {before["num_mesh_vertices"]} -> {V}, F {before["num_mesh_faces"]} -> {F}')
  gin.clear_config()
