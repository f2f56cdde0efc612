"""Field queries on the GPU (nrf_query_points / nrf_query_grid): parity with the float64 oracle's own pieces at the smallest shapes
that can go wrong, bit-identity with what the renderer saw, density-only against the full query, the grid, a query next to a stashed
training call, nrf_warp_points against the query's warped points and on a stashed call's workspace, and the Python surface down to
scripts/export_density.py.

Oracle parity, per output and per case: max error over the points / the oracle output's max-abs, against 4 x the same statistic of
the oracle evaluated in float32 on the same inputs, computed here on the CPU (the rule helpers.D_RAW_TOL documents).  The one-point
shape (1, 1) alone takes the model's pooled floor instead, the worst float32-oracle figure over the model's shapes and both levels:
the statistic of ONE point is a single rounding error, anywhere in [0, 1 ulp], and where the float32 oracle happens to land 0.06 ulp
from the float64 value (model b, coarse, sigma: 3.4e-9 against the kernel's 7.6e-8, itself 1.3 ulp of a density of 0.6) four times its
figure is below the spacing of float32 numbers.  Every case prints its two figures and its bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import helpers as H
from oracle import nerfies_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((3, 37), (70, 1), (1, 1), (2, 64))   # a ragged last tile with group boundaries inside; a new group on every row; one row; group == tile
BOX = 1.3                                      # synthetic_batch: origins in [-0.5, 0.5]^3, unit directions, z <= far = 0.826
ALPHA = 3.25

_WARP = dict(use_warp=True, num_warp_freqs=6)
MODELS = {
    'a_viewdirs_camera': dict(use_camera_metadata=True),
    'b_no_condition': dict(use_viewdirs=False),
    'c_alpha_condition': dict(use_appearance_metadata=True, use_alpha_condition=True),
    'd_narrow': dict(nerf_trunk_width=128, nerf_rgb_branch_width=64),
    'e_rgb_depth2': dict(nerf_rgb_branch_depth=2),
    'f_skip5': dict(nerf_skips=(5,)),
    'g_se3': dict(_WARP),
    'i_translation': dict(_WARP, warp_field_type='translation'),
}
_CACHE = {}


def _model(name, **more):
  """(spec, float32-rounded oracle tree in float64, model, FlatParams), built once per model."""
  key = (name, tuple(sorted(more.items())))
  if key not in _CACHE:
    spec = O.ModelSpec(**MODELS[name], **more)
    p = O.init_params(spec, seed=11 + len(name), trained_like=True)
    model, fp = H.gpu_model(spec, p)
    _CACHE[key] = (spec, O.tree_map(lambda t: t.float().double() if t.is_floating_point() else t, p), model, fp)
  return _CACHE[key]


def _inputs(spec, G, S, seed):
  """float32 points in the samples' box, unit view directions and ids, one row per group."""
  g = torch.Generator().manual_seed(seed)
  pts = ((torch.rand(G, S, 3, generator=g) * 2 - 1) * BOX).float()
  vd = torch.randn(G, 3, generator=g)
  vd = (vd / vd.norm(dim=-1, keepdim=True)).float()
  md = {'warp': torch.randint(0, spec.num_warp_embeddings, (G, 1), generator=g),
        'appearance': torch.randint(0, spec.num_appearance_embeddings, (G, 1), generator=g),
        'camera': torch.randint(0, spec.num_camera_embeddings, (G, 1), generator=g)}
  return pts, vd, md


def _oracle(p, spec, level, pts, vd, md, use_warp, metadata_encoded, dtype):
  """render_samples up to the activations (models.py:230-277) from the oracle's own pieces, in `dtype`."""
  cast = lambda t: t.to(dtype) if t.is_floating_point() else t
  p = O.tree_map(cast, p)
  pts, vd = pts.to(dtype), vd.to(dtype)
  md = {k: cast(v) for k, v in md.items()}
  alpha_c, rgb_c = O.get_condition_inputs(p, spec, vd, md, metadata_encoded)
  out = {}
  x = pts
  if use_warp:
    wm = md['warp']
    wm = wm[:, None, :].expand(pts.shape[0], pts.shape[1], wm.shape[-1])
    x = O.se3_field(p['warp_field'], pts, wm, ALPHA, spec.num_warp_freqs, False, metadata_encoded)['warped_points']
    out['warped_points'] = x
  raw_rgb, raw_alpha = O.nerf_mlp(p[f'nerf_mlps_{level}'], O.sinusoidal_encode(x, spec.num_nerf_point_freqs), alpha_c, rgb_c, spec)
  out['rgb'] = torch.sigmoid(raw_rgb)
  out['sigma'] = O._sigma_act(spec.sigma_activation, raw_alpha[..., 0])
  return out


def _md_gpu(md, spec, names):
  return {k: md[k].to(H.DEV) for k in names}


def _md_names(spec, use_warp):
  names = []
  if spec.use_warp and use_warp:
    names.append('warp')
  if spec.use_appearance_metadata:
    names.append('appearance')
  if spec.use_camera_metadata:
    names.append('camera')
  return names


def _stat(got, ref):
  return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def _parity(name, use_warp=True, encoded=False):
  spec, p, model, fp = _model(name)
  warp_on = spec.use_warp and use_warp
  rows = []
  for level in ('coarse', 'fine'):
    for G, S in SHAPES:
      pts, vd, md = _inputs(spec, G, S, seed=1000 * G + S)
      names = _md_names(spec, use_warp)
      md_o = dict(md)
      md_g = _md_gpu(md, spec, names)
      if encoded:   # metadata_encoded: the codes themselves (the model has the warp table alone)
        assert names == ['warp']
        codes = p['warp_field']['metadata_encoder']['embed']['embedding'][md['warp'][:, 0]]
        md_o = {'warp': codes}
        md_g = {'warp': codes.float().to(H.DEV)}
      ref = _oracle(p, spec, level, pts, vd, md_o, warp_on, encoded, torch.float64)
      f32 = _oracle(p, spec, level, pts, vd, md_o, warp_on, encoded, torch.float32)
      outputs = ('sigma', 'rgb') + (('warped_points',) if warp_on else ())
      got = model.query_points(fp, pts.to(H.DEV), viewdirs=vd.to(H.DEV), metadata=md_g, warp_extra={'alpha': ALPHA}, level=level,
                               use_warp=use_warp, metadata_encoded=encoded, outputs=outputs)
      for k in ('sigma', 'rgb'):
        assert tuple(got[k].shape) == tuple(ref[k].shape)
        err, floor = _stat(got[k].cpu(), ref[k]), _stat(f32[k], ref[k])
        rows.append((level, G, S, k, err, floor))
      if warp_on:   # the bound tests/test_gpu_reference_onehop.py holds warped points to
        np.testing.assert_allclose(got['warped_points'].cpu().numpy(), ref['warped_points'].numpy(), atol=1e-4, err_msg=f'{name} {level} {G}x{S}')
  tag = name + ('' if use_warp else ' NO_WARP') + (' codes' if encoded else '')
  # Every shape with more than one point is held to its OWN float32 floor: 4 x the float32 oracle's statistic on the same inputs.
  # The (1, 1) shape alone takes the model's pooled floor -- the worst float32-oracle figure over this model's shapes and both levels:
  # the statistic of ONE point is a single rounding error, anywhere in [0, 1 ulp], and a float32 oracle that happens to land 0.06 ulp
  # from the float64 value sets a bound below the spacing of float32 numbers, which no float32 evaluation can be asked to meet
  pooled = {k: max(f for _, _, _, kk, _, f in rows if kk == k) for k in ('sigma', 'rgb')}
  bound = lambda G, S, k, floor: 4.0 * (pooled[k] if G * S == 1 else floor)
  for level, G, S, k, err, floor in rows:
    print(f'[field query parity] {tag:28s} {level:6s} ({G:2d},{S:2d}) {k:5s} gpu {err:.3e}  float32 oracle {floor:.3e}  '
          f'bound {bound(G, S, k, floor):.3e}' + ('  (pooled floor)' if G * S == 1 else ''))
  for level, G, S, k, err, floor in rows:
    assert err <= bound(G, S, k, floor), (tag, level, G, S, k, err, floor, pooled[k])


@pytest.mark.parametrize('name', sorted(MODELS))
def test_oracle_parity(name):
  _parity(name)


def test_oracle_parity_with_warp_codes():
  _parity('g_se3', encoded=True)


def test_oracle_parity_under_no_warp():
  """model h: the SE3 model queried at canonical points."""
  _parity('g_se3', use_warp=False)


def _f32(words):
  return torch.from_numpy(words.view('float32').copy())


@pytest.mark.parametrize('name', ['a_viewdirs_camera', 'g_se3'])
def test_the_query_is_what_the_renderer_saw(name):
  spec, p, model, fp = _model(name, num_coarse_samples=16, num_fine_samples=16)
  B = 5
  batch = O.synthetic_batch(B, seed=5, dtype=torch.float32)
  gb = H.gpu_batch(batch)
  out = model.apply(fp, gb, {'alpha': ALPHA}, return_points=True, return_weights=True)
  ws = model.last_call.ws
  torch.cuda.synchronize()
  o, d = batch['origins'], batch['directions']
  names = _md_names(spec, True)
  md = {k: gb['metadata'][k] for k in names}
  for lv, level, S in ((0, 'coarse', 16), (1, 'fine', 32)):
    z = _f32(H._ws_words(model, ws, 'z', lv, B * S)).reshape(B, S)
    out4 = _f32(H._ws_words(model, ws, 'out4', lv, B * S * 4)).reshape(B, S, 4)
    # the renderer's o + z d is ONE rounding: hipcc defines __fmul_rn / __fadd_rn as the plain operators and contracts the pair into a
    # fused multiply-add (v_fmac_f32 in the chains' prologue).  The float32 product is exact in float64, so this is that fma
    pts = (o.double()[:, None, :] + z.double()[..., None] * d.double()[:, None, :]).float()
    outputs = ('sigma', 'rgb') + (('warped_points',) if spec.use_warp else ())
    got = model.query_points(fp, pts.to(H.DEV), viewdirs=gb['directions'], metadata=md, warp_extra={'alpha': ALPHA}, level=level, outputs=outputs)
    assert torch.equal(got['sigma'].cpu(), out4[..., 3]), (name, level)
    assert torch.equal(got['rgb'].cpu(), out4[..., :3]), (name, level)
    if spec.use_warp:
      wp = _f32(H._ws_words(model, ws, 'wpoints', lv, B * S * 3)).reshape(B, S, 3)
      assert torch.equal(got['warped_points'].cpu(), wp), (name, level)
      assert torch.equal(got['warped_points'], out[level]['warped_points'])


@pytest.mark.parametrize('name', ['a_viewdirs_camera', 'c_alpha_condition', 'g_se3'])
def test_density_only_equals_the_full_query(name):
  spec, p, model, fp = _model(name)
  for level in ('coarse', 'fine'):
    for G, S in ((3, 37), (70, 1)):
      pts, vd, md = _inputs(spec, G, S, seed=7 * G + S)
      kw = dict(viewdirs=vd.to(H.DEV), metadata=_md_gpu(md, spec, _md_names(spec, True)), warp_extra={'alpha': ALPHA}, level=level)
      full = model.query_points(fp, pts.to(H.DEV), outputs=('sigma', 'rgb'), **kw)
      dens = model.query_points(fp, pts.to(H.DEV), outputs=('sigma',), **kw)
      again = model.query_points(fp, pts.to(H.DEV), outputs=('sigma',), **kw)
      assert torch.isfinite(full['sigma']).all() and float(full['sigma'].abs().max()) > 0
      assert torch.equal(dens['sigma'], full['sigma']), (name, level, G, S)
      assert torch.equal(again['sigma'], dens['sigma'])
      full2 = model.query_points(fp, pts.to(H.DEV), outputs=('sigma', 'rgb'), **kw)
      assert torch.equal(full2['sigma'], full['sigma']) and torch.equal(full2['rgb'], full['rgb'])
  if name == 'c_alpha_condition':   # the density-only query reads no view direction (the alpha head's condition is the appearance code)
    kw.pop('viewdirs')
    assert torch.equal(model.query_points(fp, pts.to(H.DEV), outputs=('sigma',), **kw)['sigma'], dens['sigma'])


@pytest.mark.parametrize('name', ['a_viewdirs_camera', 'g_se3'])
def test_grid(name):
  from nerfies_amd import evaluation
  spec, p, model, fp = _model(name)
  dims = (5, 3, 7)
  lo, hi = (-0.9, -0.35, 0.1), (0.6, 0.55, 1.15)
  step = [(h - l) / r for l, h, r in zip(lo, hi, dims)]
  origin = [l + 0.5 * s for l, s in zip(lo, step)]
  n = torch.arange(105)
  idx = torch.stack([n % 5, (n // 5) % 3, n // 15], -1).float()
  pts = torch.tensor(origin, dtype=torch.float32) + idx * torch.tensor(step, dtype=torch.float32)   # fl(origin + fl(idx * step))
  warp_id = 2 if spec.use_warp else None
  md = {'camera': torch.tensor([[1]], dtype=torch.int32, device=H.DEV)} if spec.use_camera_metadata else {}
  if spec.use_warp:
    md['warp'] = torch.tensor([[warp_id]], dtype=torch.int32, device=H.DEV)
  vd = torch.tensor([[0.0, 0.6, 0.8]], device=H.DEV)
  kw = dict(viewdirs=vd, metadata=md, warp_extra={'alpha': ALPHA}, level='fine')
  ref = model.query_points(fp, pts.to(H.DEV)[None], outputs=('sigma', 'rgb'), **kw)
  new = lambda c: {'sigma': torch.empty(c, device=H.DEV), 'rgb': torch.empty(c, 3, device=H.DEV)}
  whole = model.query_grid(fp, origin, step, dims, 0, 105, new(105), **kw)
  assert torch.equal(whole['sigma'], ref['sigma'][0]) and torch.equal(whole['rgb'], ref['rgb'][0])
  a = model.query_grid(fp, origin, step, dims, 0, 64, new(64), **kw)
  b = model.query_grid(fp, origin, step, dims, 64, 41, new(41), workspace_points=64, **kw)
  assert torch.equal(torch.cat([a['sigma'], b['sigma']]), whole['sigma']) and torch.equal(torch.cat([a['rgb'], b['rgb']]), whole['rgb'])
  dens = model.query_grid(fp, origin, step, dims, 0, 105, {'sigma': torch.empty(105, device=H.DEV)}, **kw)
  assert torch.equal(dens['sigma'], whole['sigma'])
  # evaluation.density_grid: the same box at its voxel centres, (X, Y, Z) with x fastest, whole and in ragged chunks
  for chunk in (1 << 21, 32):
    vol = evaluation.density_grid(model, fp, lo, hi, dims, level='fine', warp_id=warp_id, warp_extra={'alpha': ALPHA}, chunk=chunk)
    assert tuple(vol.shape) == dims and vol.stride() == (1, 5, 15) and vol.dtype == torch.float32 and vol.is_cuda
    assert torch.equal(vol.permute(2, 1, 0).reshape(-1), whole['sigma'])
    assert float(vol[4, 2, 6]) == float(whole['sigma'][104]) and float(vol[1, 0, 0]) == float(whole['sigma'][1])
  if spec.use_warp:   # the canonical volume is the NO_WARP query of the same points
    can = evaluation.density_grid(model, fp, lo, hi, dims, warp_extra={'alpha': ALPHA})
    ref0 = model.query_points(fp, pts.to(H.DEV)[None], outputs=('sigma',), use_warp=False, **kw)
    assert torch.equal(can.permute(2, 1, 0).reshape(-1), ref0['sigma'][0]) and not torch.equal(ref0['sigma'][0], whole['sigma'])


def test_a_query_leaves_a_stashed_training_call_alone():
  spec, p, model, fp = _model('g_se3', num_coarse_samples=16, num_fine_samples=16)
  B = 37
  gb = H.gpu_batch(O.synthetic_batch(B, seed=8, dtype=torch.float32))
  gen = torch.Generator().manual_seed(3)
  d_c, d_f = torch.randn(B, 3, generator=gen).to(H.DEV), torch.randn(B, 3, generator=gen).to(H.DEV)
  pts, vd, md = _inputs(spec, 3, 37, seed=2)

  def run(with_query):
    out = model.apply(fp, gb, {'alpha': ALPHA}, train=True)
    rgb = out['fine']['rgb'].clone()
    if with_query:
      q = model.query_points(fp, pts.to(H.DEV), viewdirs=vd.to(H.DEV), metadata=_md_gpu(md, spec, ['warp']), warp_extra={'alpha': 1.5},
                             level='coarse', outputs=('sigma', 'rgb', 'warped_points'))
      assert torch.isfinite(q['sigma']).all()
      model.query_points(fp, pts.to(H.DEV), metadata=_md_gpu(md, spec, ['warp']), warp_extra={'alpha': 1.5}, outputs=('sigma',))
    return rgb, model.backward(fp, gb, d_c, d_f).clone()

  rgb0, g0 = run(False)
  rgb1, g1 = run(True)
  rgb2, g2 = run(False)
  assert torch.equal(rgb0, rgb1) and float(g0.abs().max()) > 0
  # float atomics in the per-ray sums: two plain runs need not agree bitwise either; the query must move nothing beyond that
  tol = 1e-6 * float(g0.abs().max())
  print(f'[field query / stash] max |g_query - g_plain| {float((g1 - g0).abs().max()):.3e}, plain rerun {float((g2 - g0).abs().max()):.3e}, tol {tol:.3e}')
  assert float((g1 - g0).abs().max()) <= tol


@pytest.mark.parametrize('trunk', [{}, dict(warp_trunk_depth=4, warp_trunk_width=64)], ids=['se3', 'warp_trunk4x64'])
def test_warp_points_equal_the_querys_warped_points(trunk):
  """nrf_warp_points and a query of one point per group run the same SE3 kernel on explicit points with one id per point, and a
  row's value does not depend on the grid: bit for bit.  N: one row, one row past a tile, past one tile per CU pair.  The 4 x 64
  trunk runs both entries on the padded parameter image."""
  spec, p, model, fp = _model('g_se3', **trunk)
  for N in (1, 65, 4097):
    g = torch.Generator().manual_seed(31 + N)
    pts = ((torch.rand(N, 3, generator=g) * 2 - 1) * BOX).float().to(H.DEV)
    ids = torch.randint(0, spec.num_warp_embeddings, (N,), generator=g).to(H.DEV)
    direct = model.warp_points(fp, pts, ids, {'alpha': ALPHA})
    query = model.query_points(fp, pts[:, None, :], metadata={'warp': ids[:, None]}, warp_extra={'alpha': ALPHA}, outputs=('warped_points',))
    assert tuple(direct.shape) == (N, 3) and tuple(query['warped_points'].shape) == (N, 1, 3)
    assert torch.isfinite(direct).all() and not torch.equal(direct, pts)
    assert torch.equal(direct, query['warped_points'][:, 0]), (trunk, N)


def test_warp_points_on_a_stashed_workspace_forgets_the_stash():
  """nrf_warp_points writes its tables and images at the start of the memory it is handed.  Handed the workspace of a stashed
  nrf_forward(NRF_FLAG_TRAIN) it forgets that stash (as a query does): nrf_backward is refused instead of differentiating what was
  written over, and the next forward uploads its tables again."""
  from nerfies_amd import lib as L, models as M
  spec, p, model, fp = _model('g_se3', num_coarse_samples=16, num_fine_samples=16)
  B, n = 5, 3
  gb = H.gpu_batch(O.synthetic_batch(B, seed=9, dtype=torch.float32))
  gen = torch.Generator().manual_seed(6)
  d_c, d_f = torch.randn(B, 3, generator=gen).to(H.DEV), torch.randn(B, 3, generator=gen).to(H.DEV)
  pts = ((torch.rand(n, 3, generator=gen) * 2 - 1) * BOX).float().to(H.DEV)
  ids = torch.tensor([2, 0, 1], dtype=torch.int32, device=H.DEV)

  def forward():
    return model.apply(fp, gb, {'alpha': ALPHA}, train=True)['fine']['rgb'].clone()

  rgb0 = forward()
  g0 = model.backward(fp, gb, d_c, d_f).clone()
  assert float(g0.abs().max()) > 0
  forward()
  ws = model.stash.ws
  need = C.c_size_t(0)
  L.check(model.lib.nrf_warp_points_workspace_bytes(model.handle, n, C.byref(need)), model.lib)
  assert need.value < ws.numel() * 4                         # every call below is in bounds
  warped = torch.empty(n, 3, device=H.DEV)
  scal = M._scalars({'alpha': ALPHA})
  L.check(model.lib.nrf_warp_points(model.handle, M._ptr(fp.flat), M._ptr(pts), M._ptr(ids), n, C.byref(scal), M._ptr(warped), M._ptr(ws),
                                    ws.numel() * 4, M._stream(H.DEV)), model.lib)
  assert torch.equal(warped, model.warp_points(fp, pts, ids, {'alpha': ALPHA}))   # the same call on memory of its own
  with pytest.raises(L.NrfError, match='error -6'):          # NRF_E_STATE
    model.backward(fp, gb, d_c, d_f)
  rgb1 = forward()
  g1 = model.backward(fp, gb, d_c, d_f)
  assert torch.equal(rgb1, rgb0)
  # float atomics in the per-ray sums: two plain runs need not agree bitwise (test_a_query_leaves_a_stashed_training_call_alone)
  tol = 1e-6 * float(g0.abs().max())
  print(f'[warp points / stash] max |g_after - g_plain| {float((g1 - g0).abs().max()):.3e}, tol {tol:.3e}')
  assert float((g1 - g0).abs().max()) <= tol


def test_python_surface_shapes_and_null_outputs():
  spec, p, model, fp = _model('g_se3')
  pts, vd, md = _inputs(spec, 6, 5, seed=4)
  mdg = _md_gpu(md, spec, ['warp'])
  one = model.query_points(fp, pts[0].to(H.DEV), viewdirs=vd[:1].to(H.DEV), metadata={'warp': mdg['warp'][:1]}, warp_extra={'alpha': ALPHA})
  assert set(one) == {'sigma', 'rgb'} and tuple(one['sigma'].shape) == (5,) and tuple(one['rgb'].shape) == (5, 3)   # (N, 3): one group
  gs = model.query_points(fp, pts.to(H.DEV), viewdirs=vd.to(H.DEV), metadata=mdg, warp_extra={'alpha': ALPHA},
                          outputs=('sigma', 'rgb', 'warped_points'))
  assert tuple(gs['sigma'].shape) == (6, 5) and tuple(gs['rgb'].shape) == (6, 5, 3) and tuple(gs['warped_points'].shape) == (6, 5, 3)
  assert torch.equal(gs['sigma'][0], one['sigma']) and torch.equal(gs['rgb'][0], one['rgb'])      # a row does not depend on its launch
  lead = model.query_points(fp, pts.reshape(2, 3, 5, 3).to(H.DEV), viewdirs=vd.reshape(2, 3, 3).to(H.DEV),
                            metadata={'warp': mdg['warp'].reshape(2, 3, 1)}, warp_extra={'alpha': ALPHA})
  assert tuple(lead['sigma'].shape) == (2, 3, 5) and torch.equal(lead['sigma'].reshape(6, 5), gs['sigma'])
  # the outputs selection reaches the library as NULL pointers
  seen = []
  real = model.lib

  class Spy:
    def __getattr__(self, k):
      return getattr(real, k)

    def nrf_query_points(self, *a):
      fo = a[8]._obj
      seen.append((fo.sigma is not None, fo.rgb is not None, fo.warped_points is not None))
      return real.nrf_query_points(*a)

  model._lib = Spy()
  try:
    for outputs in (('sigma',), ('rgb',), ('warped_points',), ('sigma', 'warped_points'), ('sigma', 'rgb', 'warped_points')):
      got = model.query_points(fp, pts.to(H.DEV), viewdirs=vd.to(H.DEV), metadata=mdg, warp_extra={'alpha': ALPHA}, outputs=outputs)
      assert set(got) == set(outputs)
      for k in outputs:
        assert torch.equal(got[k], gs[k]), (outputs, k)
  finally:
    model._lib = real
  assert seen == [(True, False, False), (False, True, False), (False, False, True), (True, False, True), (True, True, True)]
  from nerfies_amd import lib as L
  with pytest.raises(L.NrfError, match='viewdirs'):
    model.query_points(fp, pts.to(H.DEV), metadata=mdg, warp_extra={'alpha': ALPHA})            # rgb without a view direction
  with pytest.raises(L.NrfError, match='outputs'):
    model.query_points(fp, pts.to(H.DEV), metadata=mdg, outputs=('depth',))


GIN = """
max_steps = 12
LR = {'type': 'exponential', 'initial_value': 0.002, 'final_value': 0.001, 'num_steps': %max_steps}
ExperimentConfig.image_scale = 1
ExperimentConfig.random_seed = 3
ModelConfig.num_coarse_samples = 16
ModelConfig.num_fine_samples = 16
ModelConfig.num_nerf_point_freqs = 4
ModelConfig.use_warp = True
ModelConfig.warp_field_type = 'se3'
ModelConfig.num_warp_freqs = 4
ModelConfig.use_camera_metadata = True
ModelConfig.sigma_activation = @nn.softplus
TrainConfig.batch_size = 128
TrainConfig.max_steps = %max_steps
TrainConfig.lr_schedule = %LR
TrainConfig.warp_alpha_schedule = ('linear', 0.0, 4.0, 10)
TrainConfig.print_every = 100
TrainConfig.log_every = 100
TrainConfig.save_every = 12
"""


def test_export_density_end_to_end(tmp_path):
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'scripts'))
  import train as train_driver
  import export_density
  from nerfies_amd import datasets, gin_lite as gin
  cap, exp = str(tmp_path / 'cap'), str(tmp_path / 'exp')
  datasets.write_synthetic_scene(cap, num_frames=8, size=(24, 16))
  cfg = tmp_path / 'run.gin'
  cfg.write_text(GIN)
  args = ['--base_folder', exp, '--data_dir', cap, '--gin_configs', str(cfg)]
  gin.clear_config()
  state = train_driver.main(args)
  assert state.optimizer.step == 12
  for extra, name in ((['--frame', '000002'], '000002'), (['--canonical'], 'canonical')):
    gin.clear_config()
    # the threshold sits inside the softplus density's range after a few steps: some voxels in, some out
    probe = export_density.main(args + extra + ['--resolution', '6', '5', '4', '--threshold', '1e30'])
    assert probe['num_vertices'] == 0
    grid = np.load(os.path.join(exp, f'density_{name}.npy'))
    assert grid.shape == (6, 5, 4) and grid.dtype == np.float32 and np.isfinite(grid).all() and grid.min() >= 0
    thr = float(np.sort(grid.ravel())[grid.size // 2])   # a grid value itself: `>` is exact in float32 and in float64
    gin.clear_config()
    res = export_density.main(args + extra + ['--resolution', '6', '5', '4', '--threshold', repr(thr)])
    grid2 = np.load(res['npy'])
    assert np.array_equal(grid2, grid)
    want = int((grid > thr).sum())
    assert 0 < want < grid.size and res['num_vertices'] == want
    lines = open(res['ply']).read().splitlines()
    assert lines[0] == 'ply' and f'element vertex {want}' in lines
    body = lines[lines.index('end_header') + 1:]
    assert len(body) == want
    xyz = np.array([[float(v) for v in l.split()[:3]] for l in body])
    lo, hi = res['bbox']
    assert (xyz >= lo - 1e-5).all() and (xyz <= hi + 1e-5).all()
    assert all(0 <= int(v) <= 255 for l in body for v in l.split()[3:])
  gin.clear_config()
