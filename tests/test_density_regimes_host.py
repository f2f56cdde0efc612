"""Density regimes of the gradient tests, on the CPU (tests/helpers.py density_regime; the GPU side is tests/test_gpu_density_regimes.py).

Every gradient test of the suite builds its parameters with oracle.init_params(trained_like=True): softplus densities between 0.4 and
0.8 everywhere, a fine relu density of exactly 0.  A trained scene has empty space (sigma 1e-12 .. 1e-3), surfaces (sigma in the
hundreds, the transmittance gone within a few samples) and saturated colours.  This file (a) checks that each named regime meets its
defining conditions on the float64 oracle at the shapes and seeds the GPU file uses, (b) records the stock input for what it is, and
(c) measures what float32 can deliver there: the d raw of a plain float32 torch restatement of compositing + sigmoid + the sigma
activation, by torch.autograd, against the same in float64.  The GPU tolerances (helpers.D_RAW_TOL) are 4 x those floors."""
import pytest
import torch

import helpers as H
from oracle import nerfies_oracle as O

IDS = [c[0] for c in H.D_RAW_CASES]


def _fmt(s):
  return ', '.join(f'{k} {v:.3g}' for k, v in s.items())


@pytest.mark.parametrize('cid,kw,mode', H.D_RAW_CASES, ids=IDS)
def test_regime_conditions(cid, kw, mode):
  """helpers.density_regime asserts them where it builds the tree; here they are checked again from a fresh oracle evaluation."""
  spec, B, tree, b64, stats = H.regime_case(**kw)
  heads = H._heads(tree, spec, b64)
  again = {lv: H.regime_stats(spec, heads[lv], b64['directions']) for lv in H.LEVELS}
  for lv in H.LEVELS:
    print(f'[{cid}] {lv}: {_fmt(again[lv])}')
  assert again == stats
  H.assert_regime(spec, kw['regime'], again, kw.get('sat', False))
  if kw['regime'] == 'empty':   # every value a normal float32
    for lv in H.LEVELS:
      sigma = O._sigma_act(spec.sigma_activation, heads[lv]['raw']).float()
      assert (sigma >= 1.1754944e-38).all() and torch.isfinite(sigma).all()


def test_regime_conditions_of_the_alpha_condition_model():
  spec, B, tree, b64, stats = H.regime_case('surface', alpha_cond=True)
  for lv in H.LEVELS:
    print(f'[surface, use_alpha_condition] {lv}: {_fmt(stats[lv])}')
  H.assert_regime(spec, 'surface', stats)
  assert tree['nerf_mlps_fine']['MLP_2']['logit']['kernel'].shape[0] == 64 + spec.num_appearance_features


def test_the_helper_leaves_its_input_alone_and_repeats():
  spec, B, _, b64, _ = H.regime_case('surface')
  p64 = O.init_params(spec, seed=H.REGIME_SEED, trained_like=True, dtype=torch.float64)
  before = [t.clone() for _, t in O.tree_leaves_with_path(p64)]
  state = torch.random.get_rng_state()
  a, _ = H.density_regime(p64, spec, b64, 'surface', saturated_rgb=True)
  b, _ = H.density_regime(p64, spec, b64, 'surface', saturated_rgb=True)
  assert torch.equal(state, torch.random.get_rng_state())   # no random numbers of its own
  assert all(torch.equal(x, t) for x, (_, t) in zip(before, O.tree_leaves_with_path(p64)))
  changed = []
  for (path, x), (_, y), (_, t) in zip(O.tree_leaves_with_path(a), O.tree_leaves_with_path(b), O.tree_leaves_with_path(p64)):
    assert torch.equal(x, y), path
    if not torch.equal(x, t):
      changed.append(path)
  assert sorted(changed) == sorted(f'nerf_mlps_{lv}/MLP_{m}/logit/{k}' for lv in H.LEVELS for m in (1, 2) for k in ('kernel', 'bias')), changed


@pytest.mark.parametrize('act', ['softplus', 'relu'])
def test_vacuity_record_of_the_stock_input(act):
  """What tests/test_gpu_backward_ex.py's input (B = 7, 24 + 56 samples, width 64, seed 31, trained_like) exercises: one density
  regime.  If the init changes, this says what coverage moved."""
  spec = O.ModelSpec(sigma_activation=act, **H.REGIME_SHAPE)
  p64 = O.init_params(spec, seed=31, trained_like=True, dtype=torch.float64)
  b64 = O.synthetic_batch(7, seed=32, dtype=torch.float64)
  heads = H._heads(p64, spec, b64)
  stats = {lv: H.regime_stats(spec, heads[lv], b64['directions']) for lv in H.LEVELS}
  for lv in H.LEVELS:
    print(f'[stock, {act}] {lv}: {_fmt(stats[lv])}')
  if act == 'softplus':
    for lv in H.LEVELS:
      assert 0.4 < stats[lv]['sigma_min'] and stats[lv]['sigma_max'] < 0.8, stats[lv]
      assert stats[lv]['rgb_saturated'] == 0 and stats[lv]['rays_T_lt_1e3'] == 0
    assert stats['coarse']['T_min'] > 0.5   # no ray is opaque
  else:
    assert stats['fine']['sigma_max'] == 0.0 and stats['fine']['sigma_zero'] == 1.0, stats['fine']
    assert stats['coarse']['sigma_zero'] > 0.5, stats['coarse']


def _floor(cid, kw, mode):
  spec, B, tree, b64, _ = H.regime_case(**kw)
  heads = H._heads(tree, spec, b64)
  cot = H.case_cotangents(spec, B, mode)
  rows = {}
  for lv in H.LEVELS:
    raw4 = torch.cat([heads[lv]['rgb'], heads[lv]['raw'][..., None]], -1).float()   # both precisions start from the same float32 values
    z, d = heads[lv]['z'].float(), b64['directions'].float()
    c = dict(cot[lv])
    if mode == 'loss':
      with torch.no_grad():
        c['rgb'] = 2.0 * (H.render_raw(spec, raw4.double(), z.double(), d.double())['rgb'] - b64['rgb']) / b64['rgb'].numel()
    g32, _ = H.d_raw_autograd(spec, raw4, z, d, c)
    g64, _ = H.d_raw_autograd(spec, raw4.double(), z.double(), d.double(), c)
    rows[lv] = (g32, g64)
  return rows


@pytest.mark.parametrize('cid,kw,mode', H.D_RAW_CASES, ids=IDS)
def test_float32_floor_of_d_raw(cid, kw, mode):
  """The recorded floors (helpers.D_RAW_FLOOR, 1/4 of the GPU tolerances) are what this restatement gives, and with those
  tolerances it excludes at most 1 % of a case's density elements itself."""
  floor, tol = H.D_RAW_FLOOR[kw['regime']], H.D_RAW_TOL[kw['regime']]
  for lv, (g32, g64) in _floor(cid, kw, mode).items():
    inf = kw.get('inf', True)
    e = H.d_raw_errors(g32, g64, inf)
    big = e['w_rel'][~e['w_small']]
    held, share, w_ray, c_ray = H.d_raw_summary(g32, g64, tol['w_rel'], inf)
    print(f'[{cid}] {lv}: density elementwise worst {e["w_rel"].max().item():.2e} (not excludable: {big.max().item() if big.numel() else 0.0:.2e}), '
          f'/ ray max {w_ray:.2e}; colour / ray max {c_ray:.2e}; excluded at the GPU tolerance {share:.4f}')
    assert e['w_rel'].max().item() <= floor['w_rel'] and w_ray <= floor['w_ray'] and c_ray <= floor['c_ray'], (cid, lv)
    assert share <= 0.01 and held <= tol['w_rel'], (cid, lv, share, held)
