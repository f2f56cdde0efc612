"""The inverse warp on the GPU (nrf_unwarp_points): a round trip against the float64 oracle, the reported residual and status, a row
that does not depend on its launch, the step count and the warm start, the code table, a folded field, an unwarp call next to a
stashed training call, graph capture, evaluation.animate_mesh and scripts/export_density.py --animate.

Round trip.  x0 is random in the samples' box, y = W64(x0) in the float64 oracle, the GPU solves W(x) = y from x = y.  The reference
floor of a case is max_rows |W32(x0) - W64(x0)|_2, the float32 ORACLE's forward error on the same points (the code under test plays no
part in it); the GPU's |W64(x) - y| is held to 4 x floor and |x - x0| to 4 x floor / s_min, s_min the smallest singular value of the
oracle's float64 Jacobian over the case (the rule helpers.D_RAW_TOL documents: a float32 kernel against the float32 oracle).  No row is
left out; on the CPU side the float32 oracle's own Newton iteration is held to the same two bounds on every row first."""
import os
import sys

import numpy as np
import pytest
import torch

import helpers as H
from oracle import nerfies_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = 1.3
ALPHA = 3.25
SEED = 14
SHAPES = (1, 64, 70)     # one row; one full tile; a ragged second tile
_WARP = dict(use_warp=True, num_warp_freqs=6)
# (ModelSpec arguments, the factor on the "trained-like" heads, which throw points several scene sizes away as they are)
FIELDS = {
    'se3': (dict(_WARP), 0.05),
    'translation': (dict(_WARP, warp_field_type='translation'), 0.2),
    'narrow_se3': (dict(_WARP, warp_trunk_depth=3, warp_trunk_width=64), 0.05),
    'folded': (dict(_WARP), 1.0),     # not invertible: nothing non-finite may escape, and that is all
}
_PARAMS, _GPU, _REF = {}, {}, {}


def _params(name):
  """(spec, float32-rounded oracle tree in float64) with the heads scaled as tests/bf16_reference.warp_setup scales them: no GPU."""
  if name not in _PARAMS:
    kw, head_scale = FIELDS[name]
    spec = O.ModelSpec(**kw)
    p = O.init_params(spec, seed=SEED, trained_like=True)
    wf = p['warp_field']
    heads = [wf['mlp']] if spec.warp_field_type == 'translation' else [wf[br] for br in ('branches_w', 'branches_v')]
    for hd in heads:
      for k in ('kernel', 'bias'):
        hd['logit'][k] = hd['logit'][k] * head_scale
    _PARAMS[name] = (spec, O.tree_map(lambda t: t.float().double() if t.is_floating_point() else t, p))
  return _PARAMS[name]


def _model(name):
  if name not in _GPU:
    _GPU[name] = H.gpu_model(*_params(name))
  return _GPU[name]


def _field(p, spec, x, ids, dtype, jacobian=False):
  cast = lambda t: t.to(dtype) if t.is_floating_point() else t
  with torch.no_grad():
    out = O.se3_field(O.tree_map(cast, p['warp_field']), x.to(dtype), ids[:, None], ALPHA, spec.num_warp_freqs, return_jacobian=jacobian)
  return (out['warped_points'], out['jacobian']) if jacobian else out['warped_points']


def _rows(t):
  return torch.linalg.norm(t.double(), dim=-1)


def oracle_newton(p, spec, y, ids, steps=8):
  """Newton's iteration in the float32 oracle from x = y: what a float32 solver reaches, the code under test not involved."""
  x = y.float().clone()
  for _ in range(steps):
    w, J = _field(p, spec, x, ids, torch.float32, jacobian=True)
    x = x - torch.linalg.solve(J, (w - y.float())[..., None])[..., 0]
  return x


def reference_case(name, N):
  """One case, CPU only, computed once: x0, a warp id of its own per row, y = W64(x0), the floor, s_min -- and the check that the
  float32 oracle's own Newton iteration meets both bounds on every row of it."""
  key = (name, N)
  if key not in _REF:
    spec, p = _params(name)
    g = torch.Generator().manual_seed(1000 * N + 7)
    x0 = ((torch.rand(N, 3, generator=g) * 2 - 1) * BOX).float()
    ids = torch.randint(0, spec.num_warp_embeddings, (N,), generator=g)
    y, J = _field(p, spec, x0, ids, torch.float64, jacobian=True)
    floor = float(_rows(_field(p, spec, x0, ids, torch.float32).double() - y).max())
    s_min = float(torch.linalg.svdvals(J).min())
    ref = dict(x0=x0, ids=ids, y=y, floor=floor, s_min=s_min)
    if name != 'folded':
      xo = oracle_newton(p, spec, y, ids)
      ref['oracle_res'] = float(_rows(_field(p, spec, xo, ids, torch.float64) - y).max())
      ref['oracle_dx'] = float(_rows(xo.double() - x0.double()).max())
      assert ref['oracle_res'] <= 4 * floor and ref['oracle_dx'] <= 4 * floor / s_min, (name, N, ref)
    _REF[key] = ref
  return _REF[key]


def _unwarp(name, y, ids, **kw):
  model, fp = _model(name)
  kw.setdefault('steps', 8)
  guess = kw.pop('guess', None)
  return model.unwarp_points(fp, y.float().to(H.DEV), ids.to(H.DEV), {'alpha': ALPHA}, guess=None if guess is None else guess.to(H.DEV), **kw)


def _same(a, b, what):
  for k in ('points', 'residual', 'status'):
    assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


CASES = [(f, n) for f in ('se3', 'translation', 'narrow_se3') for n in SHAPES]


@pytest.mark.parametrize('name,N', CASES, ids=[f'{f}-{n}' for f, n in CASES])
def test_round_trip_against_the_float64_oracle(name, N):
  spec, p = _params(name)
  ref = reference_case(name, N)
  floor, s_min = ref['floor'], ref['s_min']
  got = _unwarp(name, ref['y'], ref['ids'], tolerance=0.0)
  assert tuple(got['points'].shape) == (N, 3) and tuple(got['residual'].shape) == (N,) and got['status'].dtype == torch.int32
  x = got['points'].cpu()
  assert torch.isfinite(x).all()
  res = float(_rows(_field(p, spec, x, ref['ids'], torch.float64) - ref['y']).max())
  dx = float(_rows(x.double() - ref['x0'].double()).max())
  print(f'[unwarp round trip] {name:11s} N {N:2d}  |W64(x) - y| gpu {res:.3e} float32 oracle {ref["oracle_res"]:.3e} floor {floor:.3e} '
        f'bound {4 * floor:.3e}   |x - x0| gpu {dx:.3e} float32 oracle {ref["oracle_dx"]:.3e} s_min {s_min:.3f} bound {4 * floor / s_min:.3e}')
  assert res <= 4 * floor, (name, N, res, floor)
  assert dx <= 4 * floor / s_min, (name, N, dx, floor, s_min)


@pytest.mark.parametrize('name', ['se3', 'translation', 'narrow_se3'])
def test_reported_residual_and_status(name):
  model, fp = _model(name)
  ref = reference_case(name, 70)
  floor = ref['floor']
  y32 = ref['y'].float().to(H.DEV)
  for tol in (4 * floor, 0.0):
    got = _unwarp(name, ref['y'], ref['ids'], tolerance=tol)
    again = model.warp_points(fp, got['points'], ref['ids'].to(H.DEV), {'alpha': ALPHA})
    host = _rows((again - y32).cpu())
    diff = float((got['residual'].cpu().double() - host).abs().max())
    print(f'[unwarp residual] {name:11s} tolerance {tol:.3e}: max |reported - recomputed| {diff:.3e} bound {4 * floor:.3e}, '
          f'status 1 on {int((got["status"] == 1).sum())} of 70 rows')
    assert diff <= 4 * floor, (name, tol, diff)
    assert set(got['status'].unique().tolist()) <= {0, 1}
    assert torch.equal(got['status'] == 1, got['residual'] <= np.float32(tol)), (name, tol)
    if tol > 0:
      assert bool((got['status'] == 1).all()), name          # the float32 iteration reaches the floor on every row (the CPU check above)


@pytest.mark.parametrize('name', ['se3', 'narrow_se3'])
def test_a_row_does_not_depend_on_its_launch(name):
  r64, r70 = reference_case(name, 64), reference_case(name, 70)
  whole = _unwarp(name, r64['y'], r64['ids'], tolerance=0.0)
  _same(whole, _unwarp(name, r64['y'], r64['ids'], tolerance=0.0), 'two runs')
  # the rows of the 64 case inside 70 rows, six places further on: rows 58..63 land in the ragged second tile
  y = torch.cat([r70['y'][:6], r64['y']])
  ids = torch.cat([r70['ids'][:6], r64['ids']])
  moved = _unwarp(name, y, ids, tolerance=0.0)
  _same({k: v[6:] for k, v in moved.items()}, whole, 'inside 70 rows')
  for i in (0, 37, 63):
    one = _unwarp(name, r64['y'][i:i + 1], r64['ids'][i:i + 1], tolerance=0.0)
    _same(one, {k: v[i:i + 1] for k, v in whole.items()}, f'row {i} alone')


def test_step_count_and_warm_start():
  name = 'se3'
  model, fp = _model(name)
  ref = reference_case(name, 70)
  tol = 4 * ref['floor']
  g = torch.Generator().manual_seed(5)
  guess = (ref['x0'] + 0.01 * torch.randn(70, 3, generator=g)).float()
  # no round: the guess comes back bit for bit, with its own residual
  got = _unwarp(name, ref['y'], ref['ids'], steps=0, guess=guess, tolerance=tol)
  assert torch.equal(got['points'].cpu().view(torch.int32), guess.view(torch.int32))
  host = _rows((model.warp_points(fp, guess.to(H.DEV), ref['ids'].to(H.DEV), {'alpha': ALPHA}) - ref['y'].float().to(H.DEV)).cpu())
  assert float((got['residual'].cpu().double() - host).abs().max()) <= 4 * ref['floor']
  assert float(got['residual'].min()) > tol and bool((got['status'] == 0).all())   # 0.01 off: nowhere near converged
  start = _unwarp(name, ref['y'], ref['ids'], steps=0, tolerance=tol)                # no guess: the target itself
  assert torch.equal(start['points'].cpu().view(torch.int32), ref['y'].float().view(torch.int32))
  # the exact preimage as the guess: converged before the first step, returned bit for bit
  got = _unwarp(name, ref['y'], ref['ids'], guess=ref['x0'], tolerance=tol)
  assert torch.equal(got['points'].cpu().view(torch.int32), ref['x0'].view(torch.int32)) and bool((got['status'] == 1).all())
  # stopped rows do not move: more rounds change nothing once every row has converged
  a = _unwarp(name, ref['y'], ref['ids'], steps=8, tolerance=tol)
  b = _unwarp(name, ref['y'], ref['ids'], steps=16, tolerance=tol)
  assert bool((a['status'] == 1).all())
  _same(a, b, 'steps 8 against 16')
  # a warm start converges in fewer rounds than the cold one needs
  warm = _unwarp(name, ref['y'], ref['ids'], steps=2, guess=guess, tolerance=tol)
  print(f'[unwarp warm start] 2 rounds from 0.01 off: status 1 on {int((warm["status"] == 1).sum())} of 70 rows')


def test_code_table_gives_the_bits_of_the_ids():
  name = 'se3'
  spec, p = _params(name)
  model, fp = _model(name)
  ref = reference_case(name, 70)
  assert len(set(ref['ids'].tolist())) > 1
  by_id = _unwarp(name, ref['y'], ref['ids'], tolerance=0.0)
  table = p['warp_field']['metadata_encoder']['embed']['embedding'].float().to(H.DEV)
  _same(_unwarp(name, ref['y'], ref['ids'], tolerance=0.0, warp_codes=table), by_id, 'the table as codes')
  # the rows of another table, in another order: the ids index ITS rows
  perm = torch.tensor([2, 0, 3, 1])
  inv = torch.argsort(perm)
  _same(_unwarp(name, ref['y'], inv[ref['ids']], tolerance=0.0, warp_codes=table[perm.to(H.DEV)]), by_id, 'a permuted table')


def test_folded_field_returns_nothing_non_finite():
  ref = reference_case('folded', 70)
  assert ref['s_min'] < 0.1                                     # the field does fold on these points
  got = _unwarp('folded', ref['y'], ref['ids'], steps=8, max_step=0.5, tolerance=4 * ref['floor'])
  assert torch.isfinite(got['points']).all() and torch.isfinite(got['residual']).all()
  assert set(got['status'].unique().tolist()) <= {0, 1, 2}
  counts = [int((got['status'] == s).sum()) for s in (0, 1, 2)]
  print(f'[unwarp folded] s_min {ref["s_min"]:.3e}: status 0 / 1 / 2 on {counts} rows, largest residual {float(got["residual"].max()):.3e}')
  # no step longer than max_step: after 8 rounds no row is further than 4 from where it started
  assert float(_rows((got['points'] - ref['y'].float().to(H.DEV)).cpu()).max()) <= 8 * 0.5 * (1 + 1e-6)


def test_an_unwarp_call_leaves_a_stashed_training_call_alone():
  spec = O.ModelSpec(**_WARP, num_coarse_samples=16, num_fine_samples=16)
  model, fp = H.gpu_model(spec, O.init_params(spec, seed=SEED, trained_like=True))
  B = 37
  gb = H.gpu_batch(O.synthetic_batch(B, seed=8, dtype=torch.float32))
  gen = torch.Generator().manual_seed(3)
  d_c, d_f = torch.randn(B, 3, generator=gen).to(H.DEV), torch.randn(B, 3, generator=gen).to(H.DEV)
  y = ((torch.rand(70, 3, generator=gen) * 2 - 1) * 0.3).to(H.DEV)
  ids = torch.randint(0, spec.num_warp_embeddings, (70,), generator=gen).to(H.DEV)

  def run(with_unwarp):
    out = model.apply(fp, gb, {'alpha': ALPHA}, train=True)
    rgb = out['fine']['rgb'].clone()
    if with_unwarp:
      got = model.unwarp_points(fp, y, ids, {'alpha': 1.5}, steps=3, max_step=0.5)
      assert torch.isfinite(got['points']).all()
    return rgb, model.backward(fp, gb, d_c, d_f).clone()

  rgb0, g0 = run(False)
  rgb1, g1 = run(True)
  rgb2, g2 = run(False)
  assert torch.equal(rgb0, rgb1) and float(g0.abs().max()) > 0
  # float atomics in the ray path's per-ray sums: two plain runs need not agree bitwise either; the call must move nothing beyond that
  tol = 1e-6 * float(g0.abs().max())
  print(f'[unwarp / stash] max |g_unwarp - g_plain| {float((g1 - g0).abs().max()):.3e}, plain rerun {float((g2 - g0).abs().max()):.3e}, tol {tol:.3e}')
  assert float((g1 - g0).abs().max()) <= tol


def test_graph_replay_equals_eager():
  """One call captured into a hipGraph on one stream (no branch) and replayed: the eager bits."""
  name = 'se3'
  model, fp = _model(name)
  ref = reference_case(name, 70)
  y, ids = ref['y'].float().to(H.DEV), ref['ids'].to(torch.int32).to(H.DEV)
  eager = model.unwarp_points(fp, y, ids, {'alpha': ALPHA}, steps=8, tolerance=0.0)   # also sizes the cached workspace
  eager = {k: v.clone() for k, v in eager.items()}
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = model.unwarp_points(fp, y, ids, {'alpha': ALPHA}, steps=8, tolerance=0.0)
  for v in out.values():
    v.zero_()
  graph.replay()
  torch.cuda.synchronize()
  _same(out, eager, 'replay')


def test_animate_mesh():
  from nerfies_amd import evaluation
  name = 'se3'
  spec, p = _params(name)
  model, fp = _model(name)
  lo, hi = (-0.9, -0.35, 0.1), (0.6, 0.55, 1.15)
  we = {'alpha': ALPHA}
  grid = evaluation.density_grid(model, fp, lo, hi, 12, level='fine', warp_id=None, warp_extra=we)
  thr = float(grid.reshape(-1).sort().values[grid.numel() // 2])
  mesh = evaluation.extract_mesh(model, fp, lo, hi, 12, thr, level='fine', warp_id=None, warp_extra=we, colors=False)
  verts = mesh['vertices']
  V = verts.shape[0]
  assert V > 50
  wids = (1, 2)
  # the floor of THIS case: the float32 oracle's forward error at the template's vertices (the scene's scale), both frames
  vc = verts.cpu()
  floor = max(float(_rows(_field(p, spec, vc, torch.full((V,), w), torch.float32).double() - _field(p, spec, vc, torch.full((V,), w), torch.float64)).max())
              for w in wids)
  # status 1 is decided on the stash-keeping kernel's W(x); the check below recomputes W(x) with nrf_warp_points' kernel, a float32
  # forward of its own (one floor apart at most by the floor's definition): a row that stopped at 2 x floor is back within 4 x floor
  tol = 2 * floor
  out = evaluation.animate_mesh(model, fp, verts, wids, warp_extra=we, steps=8, tolerance=tol)
  assert tuple(out['vertices'].shape) == (2, V, 3) and tuple(out['residual'].shape) == (2, V) and tuple(out['status'].shape) == (2, V)
  assert out['status'].dtype == torch.int32
  for k, w in enumerate(wids):
    back = model.warp_points(fp, out['vertices'][k], torch.full((V,), w, dtype=torch.int32, device=H.DEV), we)
    ok = out['status'][k] == 1
    err = float(_rows((back - verts)[ok].cpu()).max())
    print(f'[animate_mesh] frame {w}: V {V}, status 1 on {100.0 * float(ok.double().mean()):.1f} %, max |W(x) - vertex| there {err:.3e} '
          f'floor {floor:.3e} bound {4 * floor:.3e}')
    assert bool(ok.any()) and err <= 4 * floor, (w, err, floor)
  second = model.unwarp_points(fp, verts, torch.full((V,), wids[1], dtype=torch.int32, device=H.DEV), we, guess=out['vertices'][0], steps=8,
                               tolerance=tol)
  _same({k: out[k2][1] for k, k2 in (('points', 'vertices'), ('residual', 'residual'), ('status', 'status'))}, second, 'warm start')
  cold = evaluation.animate_mesh(model, fp, verts, wids, warp_extra=we, steps=8, tolerance=tol, warm_start=False)
  _same({k: cold[k2][1] for k, k2 in (('points', 'vertices'), ('residual', 'residual'), ('status', 'status'))},
        model.unwarp_points(fp, verts, torch.full((V,), wids[1], dtype=torch.int32, device=H.DEV), we, steps=8, tolerance=tol), 'cold start')
  assert torch.equal(cold['vertices'][0], out['vertices'][0])


def test_export_density_animate_end_to_end(tmp_path, capsys):
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
  grid = np.load(export_density.main(common + ['--threshold', '1e30'])['npy'])
  thr = float(np.sort(grid.ravel())[grid.size // 2])
  gin.clear_config()
  capsys.readouterr()
  res = export_density.main(common + ['--threshold', repr(thr), '--mesh', '--animate', '000001', '000005'])
  printed = capsys.readouterr().out
  gin.clear_config()
  V, F = res['num_mesh_vertices'], res['num_mesh_faces']
  assert V > 0 and F > 0
  assert res['animated'] == {i: os.path.join(exp, f'mesh_canonical_at_{i}.ply') for i in ('000001', '000005')}
  blobs = []
  for path in (res['mesh_ply'], res['animated']['000001'], res['animated']['000005']):
    blob = open(path, 'rb').read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    head = blob[:end].decode('ascii').splitlines()
    assert f'element vertex {V}' in head and f'element face {F}' in head, path
    assert len(blob) == end + V * 27 + F * 13
    vert = np.frombuffer(blob, dtype=[('xyz', '<f4', 3), ('n', '<f4', 3), ('rgb', 'u1', 3)], count=V, offset=end)
    assert np.isfinite(vert['xyz']).all() and np.isfinite(vert['n']).all(), path
    blobs.append((vert, blob[end + V * 27:]))
  for vert, faces in blobs[1:]:
    assert faces == blobs[0][1]                                   # the template's face block, byte for byte
    assert np.array_equal(vert['rgb'], blobs[0][0]['rgb'])        # and its colours
  for item in ('000001', '000005'):
    line = [l for l in printed.splitlines() if l.startswith(f'mesh_canonical_at_{item}:')]
    assert len(line) == 1 and f'{V} vertices' in line[0] and 'converged' in line[0] and 'out of steps' in line[0], printed
