"""The SE(3) algebra of csrc/se3_math.h on the GPU, regime by regime of the rotation angle theta = |w| (helpers.rotation_regime:
'init' the reference initialisation, 'tiny', 'seam' rows on both sides of theta = 0.2 where the first version of the header switched
from series to closed forms, 'trained', 'large' rows on both sides of pi and up to 7.1).

(a) Each kernel against ITS OWN inputs.  After a training step the head outputs (w, v), the sample points, the upstream d_points and
    the kernel's results are read from the workspace (nrf_debug_ws_offset); warped points, (dw, dv) of se3_vjp and -- with the elastic
    regulariser on -- the Dual Hessian-vector products of elastic_kernel are recomputed from those alone in float64.  Nothing of the
    trunk enters, so the MLP's float32 error cannot hide a coefficient fault.  Gate: the error relative to the quantity's max-abs
    over the level is at most 4 x F, F being the same figure for a float32 torch evaluation of the same algebra with exact
    coefficients on the same inputs (tests/se3_reference.py) -- a property of float32 arithmetic, not of the kernels.
(b) What it feeds: the pinned gradient check with the elastic and background regularisers on, nrf_warp_points and the Jacobian output
    against the float64 oracle, judged on the displacement / on J - I.
(c) The other kernels that include the header: the camera delta table at |omega| on both sides of every switch, and the bf16 trunk's
    exp_se3 forward on its own inputs.

B = 7 rays of 24 + 56 samples (168 coarse rows: two 64-row tiles and a ragged third), one case of 5 rays of 64 + 128."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import se3_reference as R
from oracle import nerfies_oracle as O

pytestmark = pytest.mark.gpu

WE = {'alpha': H.ROTATION_ALPHA, 'time_alpha': 0.0}
ELASTIC = {'weight': 0.01, 'reduce_method': 'weight'}


def _buf(model, ws, name, level, n):
  from nerfies_amd import lib as L
  off = C.c_int64(0)
  L.check(model.lib.nrf_debug_ws_offset(model.handle, name.encode(), level, C.byref(off)), model.lib)
  return ws[off.value:off.value + n].cpu()


def _gate(got, ref, f32, label):
  """error / max|ref| of `got` and of the float32 floor `f32`; asserts error <= 4 F."""
  ref = ref.double()
  scale = ref.abs().max().item()
  assert scale > 0 and torch.isfinite(got).all(), label
  e = (got.double() - ref).abs().max().item() / scale
  F = (f32.double() - ref).abs().max().item() / scale
  print(f'[{label}] max-abs {scale:.3e}: error {e:.2e}, float32 floor F {F:.2e} (gate 4 F = {4 * F:.2e})')
  assert e <= 4 * F, (label, e, F)
  return e, F


def _step(regime, three=False, elastic=None, bf16=False):
  """One training step on the regime's case; the workspace it ran in."""
  spec, B, tree, b64, _ = H.rotation_case(regime, three)
  model, fp = H.gpu_model(spec, tree, B)
  el = dict(ELASTIC, loss_type=elastic) if elastic else None
  grad, stats = model.loss_and_grad(fp, H.gpu_batch(b64), warp_extra=WE, elastic=el, bf16=bf16)
  torch.cuda.synchronize()
  assert torch.isfinite(grad).all() and torch.isfinite(stats).all()
  return spec, B, model, model.workspace(B, True, H.DEV, 0, el is not None, bf16=bf16), stats.cpu()


def _rows(spec, B, level):
  return B * (spec.num_coarse_samples + (spec.num_fine_samples if level else 0))


def _own(model, ws, n, level, reverse=True):
  wv = _buf(model, ws, 'w_st_wv', level, 8 * n).reshape(n, 2, 4)
  o = dict(w=wv[:, 0, :3].contiguous(), v=wv[:, 1, :3].contiguous(), x=_buf(model, ws, 'points_raw', level, 3 * n).reshape(n, 3),
           xw=_buf(model, ws, 'wpoints', level, 3 * n).reshape(n, 3), g=_buf(model, ws, 'd_points', level, 3 * n).reshape(n, 3))
  if reverse:
    o.update(dw=_buf(model, ws, 'w_dw4', level, 4 * n).reshape(n, 4)[:, :3], dv=_buf(model, ws, 'w_dv4', level, 4 * n).reshape(n, 4)[:, :3])
  return o


def _check_forward_and_vjp(regime, label, model, ws, spec, B, extra=None, reverse=True):
  """se3_apply and se3_vjp of both levels on the kernels' own inputs; extra = (dw, dv) the coarse reverse kernel adds (elastic)."""
  for level in (0, 1):
    n = _rows(spec, B, level)
    o = _own(model, ws, n, level, reverse)
    th = torch.linalg.norm(o['w'].double(), dim=-1)
    print(f'[{label} level {level}] {n} rows, theta in [{th.min().item():.3e}, {th.max().item():.3e}] median {th.median().item():.3e}')
    z = torch.zeros_like(o['w'])
    ref = R.eval_all(o['w'], o['v'], o['x'], o['g'], z, z, z, torch.float64)
    f32 = R.eval_all(o['w'], o['v'], o['x'], o['g'], z, z, z, torch.float32)
    # the kernel returns x + delta: the floor of the displacement read back from it carries the rounding of that sum
    _gate(o['xw'].double() - o['x'].double(), ref['delta'], (o['x'] + f32['delta']).double() - o['x'].double(), f'{label} level {level} x\' - x')
    if not reverse:
      continue
    add = extra if (extra is not None and level == 0) else (0.0, 0.0)
    assert o['g'].abs().max().item() > 0
    _gate(o['dw'], ref['dw'] + add[0], (f32['dw'] + add[0]) if extra is not None and level == 0 else f32['dw'], f'{label} level {level} dw')
    _gate(o['dv'], ref['dv'] + add[1], (f32['dv'] + add[1]) if extra is not None and level == 0 else f32['dv'], f'{label} level {level} dv')


@pytest.mark.parametrize('regime', H.ROTATION_REGIMES)
def test_own_inputs_apply_and_vjp(regime):
  """se3_warp_fwd_kernel / se3_warp_bwd_kernel, elastic loss off: (dw, dv) is pure se3_vjp."""
  spec, B, model, ws, _ = _step(regime)
  _check_forward_and_vjp(regime, regime, model, ws, spec, B)


def test_own_inputs_apply_and_vjp_three_tiles_per_ray():
  spec, B, model, ws, _ = _step('seam', three=True)
  _check_forward_and_vjp('seam', 'seam 64+128', model, ws, spec, B)


def _elastic_reference(o, wd, vd, coef, B, loss_type, dtype):
  """elastic_kernel restated on its own inputs in `dtype`: E = J - I by Dual columns, dL/dJ by autograd of the oracle's
  compute_elastic_loss, its pull-back through exp_se3 by se3_vjp on Duals.  Returns dict(E, tan_dw, tan_dv (3, n, 3), el_dw, el_dv,
  rho, res, det, div, curl per row)."""
  n = o['w'].shape[0]
  eye = torch.eye(3, dtype=dtype)
  cols = [R.eval_all(o['w'], o['v'], o['x'], o['g'], wd[c], vd[c], eye[c].expand(n, 3), dtype) for c in range(3)]
  E = torch.stack([c['jcol'] for c in cols], -1)   # E[:, i, c]
  J = (eye + E).requires_grad_(True)
  rho, res = O.compute_elastic_loss(J, loss_type=loss_type)
  (coef.to(dtype) * rho).sum().mul(ELASTIC['weight'] / B).backward()
  G = J.grad
  out = dict(E=E, rho=rho.detach(), res=res.detach(), det=torch.linalg.det(J.detach()), div=O.jacobian_to_div(J.detach()),
             curl=torch.linalg.norm(O.jacobian_to_curl(J.detach()), dim=-1), tan_dw=[], tan_dv=[], el_dw=0.0, el_dv=0.0)
  for c in range(3):
    p = R.eval_all(o['w'], o['v'], o['x'], G[:, :, c], wd[c], vd[c], eye[c].expand(n, 3), dtype)
    out['tan_dw'].append(p['dw']); out['tan_dv'].append(p['dv'])
    out['el_dw'], out['el_dv'] = out['el_dw'] + p['hdw'], out['el_dv'] + p['hdv']
  out['tan_dw'], out['tan_dv'] = torch.stack(out['tan_dw']), torch.stack(out['tan_dv'])
  return out


@pytest.mark.parametrize('regime,loss_type', [(r, 'log_svals') for r in H.ROTATION_REGIMES] + [('seam', 'div'), ('large', 'det'), ('large', 'svals')])
def test_own_inputs_elastic_hessian_vector_products(regime, loss_type):
  """elastic_kernel: J - I (Dual columns), the gradient w.r.t. the head tangents (se3_vjp values on Duals) and w.r.t. the primal
  heads (its tangent parts: Hessian-vector products, where dAb / dBb / dCb enter), the loss, the residual and the Jacobian statistics;
  then the coarse reverse kernel, which adds the primal part to se3_vjp.

  What this gate can and cannot see: F is a float32 evaluation of the WHOLE of elastic_kernel's job, the singular values and the
  robust loss included, and torch's float32 svdvals + log loses digits near J = I that the kernel's log1p form keeps.  So F is 20x to
  1700x the kernel's error at 'init' and 'tiny' and about 10x at 'seam': there the 4 F gate pins the kernel's layout, scaling and
  signs, not a coefficient's last digits (the header of the parent commit passes every case, and dCb x 1.5 is caught in 'large' only,
  where F is at the kernel's own level).  The coefficients' digits are held by tests/test_se3_math_host.py, on hdw / hdv.
  'large' with log_svals and svals also runs the kernel's recomputation of small eigenvalues of J^T J as |J v|^2."""
  spec, B, model, ws, stats = _step(regime, elastic=loss_type)
  n = _rows(spec, B, 0)
  pad = (n + 63) // 64 * 64
  o = _own(model, ws, n, 0)
  tan = _buf(model, ws, 'w_st_wv', 3, 8 * 3 * pad).reshape(3, pad, 2, 4)[:, :n]
  wd, vd = tan[:, :, 0, :3].contiguous(), tan[:, :, 1, :3].contiguous()
  coef = _buf(model, ws, 'weights', 0, n)
  got = dict(tan_dw=_buf(model, ws, 'w_dw4', 3, 4 * 3 * pad).reshape(3, pad, 4)[:, :n, :3],
             tan_dv=_buf(model, ws, 'w_dv4', 3, 4 * 3 * pad).reshape(3, pad, 4)[:, :n, :3],
             el_dw=_buf(model, ws, 'el_dw4', 0, 4 * n).reshape(n, 4)[:, :3], el_dv=_buf(model, ws, 'el_dv4', 0, 4 * n).reshape(n, 4)[:, :3])
  assert wd.abs().max().item() > 0 and coef.abs().max().item() > 0
  ref = _elastic_reference(o, wd, vd, coef, B, loss_type, torch.float64)
  f32 = _elastic_reference(o, wd, vd, coef, B, loss_type, torch.float32)
  label = f'{regime} {loss_type}'
  print(f'[{label}] max |J - I| {ref["E"].abs().max().item():.3e}')
  for k in ('tan_dw', 'tan_dv', 'el_dw', 'el_dv'):
    _gate(got[k], ref[k], f32[k], f'{label} elastic {k}')
  # the statistics are means over the rows: the floor of a mean is the mean of the rows' float32 errors
  c64 = coef.double()
  for idx, name, r64, r32 in ((6, 'loss/elastic', c64 * ref['rho'] * (n / B), c64 * f32['rho'].double() * (n / B)),
                              (7, 'residual/elastic', ref['res'], f32['res'].double()), (12, 'jacobian det', ref['det'], f32['det'].double()),
                              (13, 'jacobian div', ref['div'], f32['div'].double()), (14, 'jacobian curl', ref['curl'], f32['curl'].double())):
    want, F = r64.mean().item(), (r32 - r64).abs().mean().item()
    scale = r64.abs().mean().item()
    e = abs(stats[idx].item() - want)
    print(f'[{label}] {name}: {stats[idx].item():.7e} against {want:.7e}; error / mean-abs {e / scale:.2e}, floor {F / scale:.2e}')
    assert e <= 4 * F + 2.0 ** -23 * abs(want), (label, name, e, F)   # + one rounding of the float32 figure itself
  _check_forward_and_vjp(regime, label, model, ws, spec, B, extra=(got['el_dw'].double(), got['el_dv'].double()))


# ---------------------------------------------------------------------------------------------------------------- (b)
def _background(spec, seed=7, n=32):
  g = torch.Generator().manual_seed(seed)
  return {'points': (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * 0.8,
          'warp_ids': torch.randint(0, spec.num_warp_embeddings, (n, 1), generator=g),
          'noise': 1e-3 * torch.randn(n, 3, generator=g, dtype=torch.float64), 'weight': 1.0}


@pytest.mark.parametrize('regime', H.ROTATION_REGIMES)
def test_pinned_gradients_with_elastic_and_background(regime):
  spec, B, tree, b64, _ = H.rotation_case(regime)
  r = H.run_pinned(spec, B, H.ROTATION_ALPHA, params=tree, batch=b64, elastic=dict(ELASTIC), background=_background(spec))
  H.assert_pinned(r, f'{regime} elastic + background')
  carried = {p: s for p, (e, s) in r['errs'].items() if p.startswith('warp_field/')}
  assert any('trunk' in p for p in carried) and all(s > 0 for s in carried.values()), carried
  for must in ('warp_field/branches_w/logit/kernel', 'warp_field/branches_v/logit/kernel', 'warp_field/metadata_encoder/embed/embedding'):
    assert carried[must] > 0, must


def _heads_at(tree, spec, pts, ids, dtype, split_bf16=False):
  """(w, v) of the oracle's SE3 field at pts in `dtype`; split_bf16: every dense layer as csrc/mlp_bf16x3.hip states its products,
  w x = w_hi x_hi + w_lo x_hi + w_hi x_lo with hi = bf16(.), lo = bf16(. - hi), summed in `dtype`."""
  cast = lambda t: t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t
  wf = O.tree_map(cast, tree['warp_field'])
  key = {id(wf['branches_w']['logit']): 'w', id(wf['branches_v']['logit']): 'v'}
  seen = {}

  def hook(p, x):
    if split_bf16:
      xh, kh = H.bf16_round(x), H.bf16_round(p['kernel'])
      xl, kl = H.bf16_round(x - xh), H.bf16_round(p['kernel'] - kh)
      y = ((xh @ kh + xh @ kl + xl @ kh) + p['bias']).to(p['kernel'].dtype)   # bf16_round returns float64 holding bf16 values
    else:
      y = x @ p['kernel'] + p['bias']
    if id(p) in key:
      seen[key[id(p)]] = y.detach()
    return y
  with torch.no_grad(), O.dense_hook(hook):
    O.se3_field(wf, pts.to(dtype), ids, H.ROTATION_ALPHA, spec.num_warp_freqs)
  return seen['w'], seen['v']


@pytest.mark.parametrize('regime', H.ROTATION_REGIMES)
@pytest.mark.parametrize('n', [1, 257])
def test_warp_points_displacement(regime, n):
  """nrf_warp_points at the case's own sample points against the float64 oracle, on the displacement x' - x.  The floor: the oracle's
  trunk and heads in float32, then the algebra in float32 with exact coefficients (the oracle's own normalised-axis form cancels at
  small angles and would make any gate meaningless there)."""
  spec, B, tree, b64, _ = H.rotation_case(regime)
  with torch.no_grad():
    ret = O.nerf_model_apply(tree, spec, b64, H.ROTATION_ALPHA, return_points=True)
  pts = torch.cat([ret[lv]['points'].reshape(-1, 3) for lv in H.LEVELS])
  ids = torch.cat([b64['metadata']['warp'].reshape(B, 1).expand(B, ret[lv]['points'].shape[1]).reshape(-1) for lv in H.LEVELS])
  pick = torch.arange(n) * (pts.shape[0] // n)
  pts, ids = pts[pick].float(), ids[pick].reshape(-1, 1)
  model, fp = H.gpu_model(spec, tree, B)
  got = model.warp_points({'params': fp}, pts.to(H.DEV), ids.to(H.DEV), WE).cpu()
  z = torch.zeros_like(pts)
  w64, v64 = _heads_at(tree, spec, pts, ids, torch.float64)
  w32, v32 = _heads_at(tree, spec, pts, ids, torch.float32)
  ref = R.eval_all(w64, v64, pts, z, z, z, z, torch.float64)['delta']
  f32 = R.eval_all(w32, v32, pts, z, z, z, z, torch.float32)['delta']
  with torch.no_grad():   # the restated reference is the oracle's warp
    oracle = O.se3_field(tree['warp_field'], pts.double(), ids, H.ROTATION_ALPHA, spec.num_warp_freqs)['warped_points'] - pts.double()
  assert (oracle - ref).abs().max().item() <= 1e-9 * ref.abs().max().item() + 1e-13
  _gate(got.double() - pts.double(), ref, (pts + f32).double() - pts.double(), f'{regime} warp_points n={n}')


@pytest.mark.parametrize('regime', H.ROTATION_REGIMES)
def test_jacobian_output(regime):
  """return_warp_jacobian against float64 jacfwd of the oracle: the suite's absolute 2e-4, and relative to max |J - I| (2e-4 of it,
  plus the rounding of the stored 1 + E, 2^-24, which no float32 J can avoid) -- at 'init' |J - I| is 1e-3 and the absolute gate alone
  would pass a Jacobian with one correct digit."""
  spec, B, tree, b64, _ = H.rotation_case(regime)
  model, fp = H.gpu_model(spec, tree, B)
  out = model.apply({'params': fp}, H.gpu_batch(b64), WE, return_warp_jacobian=True)
  ref = O.nerf_model_apply(tree, spec, b64, H.ROTATION_ALPHA, return_warp_jacobian=True)
  for lv in H.LEVELS:
    J, want = out[lv]['warp_jacobian'].cpu().double(), ref[lv]['warp_jacobian'].detach()
    size = (want - torch.eye(3, dtype=torch.float64)).abs().max().item()
    err = (J - want).abs().max().item()
    print(f'[{regime} {lv}] max |J - I| {size:.3e}, error {err:.2e} ({err / size:.2e} of it)')
    np.testing.assert_allclose(J.numpy(), want.numpy(), atol=2e-4)
    assert err <= 2e-4 * size + 2.0 ** -24, (regime, lv, err, size)


# ---------------------------------------------------------------------------------------------------------------- (c)
OMEGAS = (0.0, 1e-4, 0.1999, 0.2, 0.2001, 1.0, 1.9999, 2.0, 2.0001, np.pi - 1e-3, np.pi + 1e-3, 6.0)


def _hat(w):
  z = torch.zeros((), dtype=w.dtype)
  return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


@pytest.mark.parametrize('omega', OMEGAS)
def test_camera_compose_rotation(omega):
  """nrf_camera_table_compose / _backward, 8 cameras with random axes at one |omega| (both sides of 0.2, where the header used to
  switch, of 2, where it switches now, and of pi), against float64 matrix_exp and its autograd; judged on R - R0 and on d omega."""
  from nerfies_amd import camera, lib as L
  g = torch.Generator().manual_seed(int(1000 * omega) + 3)
  n = 8
  table = torch.zeros(n, L.NRF_CAMERA_ROW, dtype=torch.float64)
  for c in range(n):
    table[c, 0:9] = torch.matrix_exp(_hat(torch.randn(3, generator=g, dtype=torch.float64))).reshape(9)
  table[:, 12] = 1.0
  deltas = torch.zeros(n, L.NRF_CAMERA_DELTA_ROW, dtype=torch.float64)
  deltas[:, 0:3] = omega * torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
  t32, d32 = table.float().to(H.DEV), deltas.float().to(H.DEV).requires_grad_(True)
  t64, d64 = t32.cpu().double(), d32.detach().cpu().double().requires_grad_(True)
  d_cam = torch.zeros(n, L.NRF_CAMERA_ROW, dtype=torch.float64)
  d_cam[:, 0:9] = torch.randn(n, 9, generator=g, dtype=torch.float64)
  d_cam = d_cam.float()
  out = camera.compose_cameras(t32, d32)
  (out * d_cam.to(H.DEV)).sum().backward()
  got_R, got_dw = out.detach().cpu()[:, 0:9].reshape(n, 3, 3), d32.grad.cpu()[:, 0:3]
  R0 = t64[:, 0:9].reshape(n, 3, 3)
  want_R = torch.stack([torch.matrix_exp(_hat(d64[c, 0:3])) @ R0[c] for c in range(n)])
  (want_R * d_cam.double()[:, 0:9].reshape(n, 3, 3)).sum().backward()
  want_dw = d64.grad[:, 0:3]
  # the kernel's algebra on its own inputs: se3_delta / se3_vjp with v = 0 on the columns of R0
  w = d32.detach().cpu()[:, None, 0:3].expand(n, 3, 3).reshape(-1, 3)
  x = t32.cpu()[:, 0:9].reshape(n, 3, 3).transpose(1, 2).reshape(-1, 3)            # column j of R0
  gg = d_cam[:, 0:9].reshape(n, 3, 3).transpose(1, 2).reshape(-1, 3)
  z = torch.zeros_like(w)
  f32 = R.eval_all(w, z, x, gg, z, z, z, torch.float32)
  f_R = (x + f32['delta']).reshape(n, 3, 3).transpose(1, 2)
  f_dw = f32['dw'].reshape(n, 3, 3).sum(1)
  if omega == 0.0:
    assert torch.equal(got_R, t32.cpu()[:, 0:9].reshape(n, 3, 3))   # R = R0 exactly
  else:
    _gate(got_R.double() - R0, want_R.detach() - R0, f_R.double() - R0, f'|omega| = {omega:g} R - R0')
  _gate(got_dw, want_dw, f_dw, f'|omega| = {omega:g} d omega')


@pytest.mark.parametrize('regime', ['seam', 'init'])
def test_bf16_trunk_exp_se3_on_its_own_inputs(regime):
  """warp_bf16.hip: the trunk runs on bfloat16 operands, the algebra is float32 -- on the (w, v, x) it read, the forward meets the
  float32 gate of (a) unchanged.  Its reverse keeps (dw, dv) only as the bfloat16 operand block of the next product ("bw_dhead"):
  rounded to 8 bits they cannot be held to a float32 floor, so the reverse is left to the float32 kernels, which run the same se3_vjp.
  The split-bf16 forward (warp_bf16x3.hip, inference only) stashes no (w, v) at all and is not covered here."""
  spec, B, model, ws, _ = _step(regime, bf16=True)
  _check_forward_and_vjp(regime, f'{regime} bf16', model, ws, spec, B, reverse=False)


@pytest.mark.parametrize('regime', ['seam', 'init'])
def test_split_bf16_forward_displacement(regime):
  """warp_bf16x3.hip (inference, bf16='x3'): it stashes no (w, v), so its se3_apply cannot be held to its own inputs; its warped points
  are compared with the float64 oracle at the points it reports, on the displacement.  The floor is the construction of
  test_warp_points_displacement in this path's own number format: the oracle's trunk and heads in float32 with every product split as
  csrc/mlp_bf16x3.hip states it (hi x hi + lo x hi + hi x lo, 2^-16 per product where float32 has 2^-24), then the float32 algebra
  with exact coefficients.  Against the float32-trunk floor the kernel is at 4.7 F at 'seam' -- the trunk's arithmetic, not the
  header's.  Both sides of theta = 0.2 and theta ~ 1e-3."""
  spec, B, tree, b64, _ = H.rotation_case(regime)
  model, fp = H.gpu_model(spec, tree, B)
  out = model.apply({'params': fp}, H.gpu_batch(b64), WE, bf16='x3', return_points=True)
  for lv in H.LEVELS:
    S = out[lv]['points'].shape[1]
    pts, got = out[lv]['points'].cpu().reshape(-1, 3), out[lv]['warped_points'].cpu().reshape(-1, 3)
    ids = b64['metadata']['warp'].reshape(B, 1).expand(B, S).reshape(-1, 1)
    z = torch.zeros_like(pts)
    w64, v64 = _heads_at(tree, spec, pts, ids, torch.float64)
    w32, v32 = _heads_at(tree, spec, pts, ids, torch.float32, split_bf16=True)
    ref = R.eval_all(w64, v64, pts, z, z, z, z, torch.float64)['delta']
    f32 = R.eval_all(w32, v32, pts, z, z, z, z, torch.float32)['delta']
    _gate(got.double() - pts.double(), ref, (pts + f32).double() - pts.double(), f'{regime} split-bf16 {lv} x\' - x')
