"""The same-rounding references of tests/bf16_reference.py, held against the float64 oracle on the CPU.

For every layout of bf16_reference.MLP_LAYOUTS / WARP_LAYOUTS the "stash" is synthesised from the float64 oracle's own forward
(activations of the caller's layers, repeated over the identity layers as the plan lays them out; d raw and the trunk's dpre from
torch.autograd), and the from-stash recomputation runs with the rounding function replaced by the identity.  It is then the plain
chain rule, and must give oracle.loss_and_grad's leaves to 1e-10 of each leaf's max-abs: the layer map, the skip rows, the missing
bottleneck, the alpha head's input and the TranslationField's leaf names of the TEST code are proven here, without a GPU.  The warp
passes are the GPU test's: coarse, fine, background and -- for the SE3 fields -- the tangent pass of the elastic loss, which is written out
layer by layer here and first shown to be the oracle's own forward-mode derivative.

The negative controls mutate the reference's layout; each must break the comparison on the layouts named at the control."""
import os
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from oracle import nerfies_oracle as O  # noqa: E402
import helpers as H  # noqa: E402
import bf16_reference as R  # noqa: E402

TOL = 1e-10
_CACHE = {}


def _oracle_run(spec, p, b, **kw):
  """One float64 forward + backward of oracle.loss_fn with every Dense's (input, output) and every hidden layer's (pre, activation)
  recorded (still attached to the graph of `total`, so the loss can be differentiated with respect to any of them)."""
  leaves = list(O.tree_leaves_with_path(p))
  req = [t.detach().clone().requires_grad_(True) for _, t in leaves]
  it = iter(req)
  params_r = O.tree_map(lambda _: next(it), p)
  names = {}

  def walk(t, path):
    if 'kernel' in t:
      names[id(t)] = path
    else:
      for k, v in t.items():
        if isinstance(v, dict):
          walk(v, f'{path}/{k}' if path else k)
  walk(params_r, '')
  dense, act = {}, {}

  def dense_hook(pd, x):
    y = x @ pd['kernel'] + pd['bias']
    dense.setdefault(names[id(pd)], []).append((x, y))
    return y

  def relu_hook(name, layer, pre):
    a = torch.relu(pre)
    act[(name, layer)] = (pre, a)
    return a
  with O.dense_hook(dense_hook), O.relu_hook(relu_hook):
    total, _, ret = O.loss_fn(params_r, spec, b, **kw)
  return types.SimpleNamespace(dense=dense, act=act, total=total, ret=ret, params=params_r, req=req, paths=[path for path, _ in leaves])


def _grad_of(total, tensors):
  return [g.detach() for g in torch.autograd.grad(total, tensors, retain_graph=True)]


def _grad_of_unused(total, tensors):
  """as _grad_of, zeros for a tensor the loss does not depend on"""
  return [torch.zeros_like(t) if g is None else g.detach() for t, g in zip(tensors, torch.autograd.grad(total, tensors, retain_graph=True, allow_unused=True))]


def _mlp_case(label):
  """(spec, float64 tree, batch, {level: synthesised stash}, oracle.loss_and_grad's gradient tree) of one MLP layout"""
  if ('mlp', label) not in _CACHE:
    spec = O.ModelSpec(**dict(R.LAYOUT_SHAPE, **R.MLP_LAYOUTS[label]))
    B = R.LAYOUT_RAYS
    p = O.init_params(spec, seed=3, trained_like=True, dtype=torch.float64)
    b = O.synthetic_batch(B, seed=4, dtype=torch.float64)
    g = torch.Generator().manual_seed(5)
    kw = dict(warp_alpha=R.WARP_ALPHA, t_rand=torch.rand(B, spec.num_coarse_samples, generator=g).double(),
              u=torch.rand(B, spec.num_fine_samples, generator=g).double())
    _, _, ograds, _ = O.loss_and_grad(p, spec, b, **kw)
    # (ray origins that require a gradient: the posenc is then a node of the graph whether or not a warp field sits in front of it)
    run = _oracle_run(spec, p, dict(b, origins=b['origins'].clone().requires_grad_(True)), **kw)
    dense, act = run.dense, run.act
    lay = R.MlpLayout(spec)   # the layout the plan gives this model: what the synthesised stash follows
    stashes = {}
    for lname in ('coarse', 'fine'):
      base = f'nerf_mlps_{lname}'
      hcall = [act[(f'{lname}/MLP_0', e)][1].detach() for e in range(spec.nerf_trunk_depth)]
      h = []
      for c in range(R.TRUNK_DEPTH):   # an identity layer repeats the activation in front of it
        h.append(hcall[lay.caller_of[c]] if lay.caller_of[c] >= 0 else h[c - 1])
      raw_rgb, raw_sig = dense[f'{base}/MLP_1/logit'][0][1], dense[f'{base}/MLP_2/logit'][0][1]
      pe = dense[f'{base}/MLP_0/hidden_0'][0][0]   # the tensor the skip layer concatenates as well (oracle.mlp: inputs = x)
      d_rgb, d_sig, d_pe = _grad_of(run.total, [raw_rgb, raw_sig, pe])
      st = dict(pe=pe.detach().reshape(-1, lay.P), d_pe=d_pe.reshape(-1, lay.P), h=h,
                bn=dense[f'{base}/bottleneck'][0][1].detach() if f'{base}/bottleneck' in dense else h[7],
                rgbh=act[(f'{lname}/MLP_1', 0)][1].detach(), draw=torch.cat([d_rgb, d_sig], -1))
      if lay.A:
        st['code'] = p['appearance_encoder']['embed']['embedding'][b['metadata']['appearance'][:, 0].long()]
        st['dsig_ray'] = d_sig.reshape(B, -1).sum(1, keepdim=True)
      stashes[lname] = st
    _CACHE[('mlp', label)] = (spec, p, b, stashes, ograds)
  return _CACHE[('mlp', label)]


def _mlp_check(label, **mutation):
  """the worst leaf error of the from-stash recomputation under the layout MlpLayout(spec, **mutation)"""
  spec, p, b, stashes, ograds = _mlp_case(label)
  lay = R.MlpLayout(spec, **mutation)
  worst = 0.0
  for lname, st in stashes.items():
    want, aux = R.mlp_leaves_from_stash(lay, p[f'nerf_mlps_{lname}'], st, R.exact, st.get('code'), st.get('dsig_ray'))
    errs = R.compare_leaves(want, ograds[f'nerf_mlps_{lname}'], lay.tw)
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, (label, lname, bad)
    # d posenc (what d_points is the chain rule of): through layer 0 and through the skip layer's posenc rows
    err = (aux['dpe'] - st['d_pe']).abs().max().item() / st['d_pe'].abs().max().item()
    assert err < TOL, (label, lname, 'd posenc', err)
    worst = max(worst, max(errs.values()), err)
  return worst


@pytest.mark.parametrize('label', list(R.MLP_LAYOUTS))
def test_mlp_reference_is_the_chain_rule_on_every_layout(label):
  spec = _mlp_case(label)[0]
  lay = R.MlpLayout(spec)
  # the cases are what their names say
  assert len(lay.identities) == R.TRUNK_DEPTH - spec.nerf_trunk_depth
  if lay.skip >= 0:
    assert lay.chain_of[lay.skip] == R.SKIP       # a skip the trunk reaches runs at the chain's skip layer
  worst = _mlp_check(label)
  print(f'[{label}] identities {lay.identities}, bottleneck {lay.bottleneck}, A {lay.A}: worst leaf {worst:.1e}')


RELAID = ('skip2-depth6-warp', 'skip1-depth5', 'skip3-depth5-noviewdirs')
NO_CONDITION = ('depth2-nocond', 'skip3-depth5-noviewdirs')
# (mutation of the reference's layout, the layouts it must break).  Everywhere else the mutation changes nothing the layout uses, and
# the comparison must still hold: a control that fails everywhere shows nothing.
CONTROLS = {
    # the caller's layers in place (chain layer = caller's layer), as if nrf_create did not move the trunk around layer 4: wrong on the
    # RELAID layouts (the stash has the identities between the caller's layers); every other layout is laid out in place anyway
    'in-place layer map': (lambda spec: dict(layer_map=list(range(spec.nerf_trunk_depth))), RELAID),
    # the posenc rows taken from layer 4 of the CALLER'S numbering: wrong on the RELAID layouts, whose layer 4 is an ordinary layer
    # (tw rows) and whose skip layer 1..3 holds them; the layouts with nerf_skips = (4,) agree with it, and a trunk of fewer than five
    # layers has no layer 4 and no posenc rows either way
    'posenc rows at the caller\'s layer 4': (lambda spec: dict(skip_rows_at=4), RELAID),
    # a bottleneck layer between the trunk and the heads: wrong on the layouts WITHOUT ANY CONDITION, whose tree has no such leaf
    'bottleneck kept': (lambda spec: dict(bottleneck=True), NO_CONDITION),
}


@pytest.mark.parametrize('label', list(R.MLP_LAYOUTS))
@pytest.mark.parametrize('control', list(CONTROLS))
def test_mlp_reference_negative_controls(control, label):
  mutate, breaks = CONTROLS[control]
  spec = _mlp_case(label)[0]
  if label in breaks:
    with pytest.raises(AssertionError):
      _mlp_check(label, **mutate(spec))
  else:
    _mlp_check(label, **mutate(spec))


def test_dense_hook_tells_the_rgb_hidden_layer_by_identity():
  """Equal trunk and rgb widths: the rgb hidden layer [tw + R, rw] still rounds only its bottleneck rows (the old shape test took
  every row); every other layer rounds all of its rows."""
  spec = O.ModelSpec(**dict(R.LAYOUT_SHAPE, **R.MLP_LAYOUTS['w128-rgb128']))
  p = O.init_params(spec, seed=3, trained_like=True, dtype=torch.float64)
  hook = R.bf16_dense_for(spec, p)
  tw = spec.nerf_trunk_width
  x = torch.randn(7, tw + spec.rgb_cond_width, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
  q = H.bf16_round
  prev, O._SCOPE = O._SCOPE, 'nerf_mlp'
  try:
    pd = p['nerf_mlps_coarse']['MLP_1']['hidden_0']
    want = q(x[:, :tw]) @ q(pd['kernel'][:tw]) + x[:, tw:] @ pd['kernel'][tw:] + pd['bias']
    assert torch.equal(hook(pd, x), want)
    pd = p['nerf_mlps_coarse']['MLP_2']['logit']
    want = q(x[:, :tw]) @ q(pd['kernel']) + pd['bias']
    assert torch.equal(hook(pd, x[:, :tw]), want)
    pd = p['nerf_mlps_coarse']['MLP_0']['hidden_1']
    assert torch.equal(hook(pd, x[:, :tw]), q(x[:, :tw]) @ q(pd['kernel']) + pd['bias'])
  finally:
    O._SCOPE = prev


# ---------------------------------------------------------------------------------------------
# warp trunk
# ---------------------------------------------------------------------------------------------
ELASTIC_WEIGHT = 0.01


def _se3_of_heads(w, v, x):
  """warping.py:338-353 behind the two head layers: the raw (w, v) of a point and the point -> the warped point"""
  theta = torch.linalg.norm(w, dim=-1)
  transform = O.exp_se3(torch.cat([w / theta[..., None], v / theta[..., None]], -1), theta)
  return O.from_homogenous((transform @ O.to_homogenous(x)[..., None])[..., 0])


def _tangent_pass(lay, spec, run, x, code, masks, wv, weights_el):
  """The forward-mode pass of the elastic loss over the coarse samples, written out layer by layer on the parameters of `run` (the
  oracle differentiates se3_warp as a whole: jax.jacfwd, warping.py:385-387): per coordinate c the tangent of the trunk input, of
  every pre-activation (the primal ReLU pattern `masks` is its derivative) and of the heads, then column c of the Jacobian through
  the SE3 algebra at the PRIMAL (w, v) `wv`.  Returns (elastic loss term, [per c: dict(X, pre [depth], h [depth], heads [2])])."""
  wf = run.params['warp_field']
  encode = lambda pts: torch.cat([O.annealed_sinusoidal_encode(pts, lay.F, R.ALPHA), code], -1)
  cols, recs = [], []
  for c in range(3):
    e = torch.zeros_like(x)
    e[:, c] = 1.0
    tX = torch.autograd.functional.jvp(encode, (x,), (e,))[1].detach()
    t, pres, hs = tX, [], []
    for l in range(lay.depth):
      Wl = wf['trunk'][f'hidden_{l}']['kernel']
      pre = t @ Wl[:t.shape[1]] + (tX @ Wl[lay.width:] if l == R.SKIP else 0)
      t = pre * masks[l]
      pres.append(pre)
      hs.append(t)
    heads = [t @ wf['branches_w']['logit']['kernel'], t @ wf['branches_v']['logit']['kernel']]
    col = torch.autograd.functional.jvp(_se3_of_heads, (wv[0], wv[1], x), (heads[0], heads[1], e), create_graph=True)[1]
    cols.append(col)
    recs.append(dict(X=tX, pre=pres, h=hs, heads=heads))
  jac = torch.stack(cols, -1).reshape(weights_el.shape + (3, 3))
  el, _ = O.compute_elastic_loss(jac)
  return ELASTIC_WEIGHT * (weights_el * el).sum(-1).mean(), recs


@pytest.mark.parametrize('label', list(R.WARP_LAYOUTS))
def test_warp_reference_is_the_chain_rule_on_every_layout(label):
  spec = O.ModelSpec(**dict(R.LAYOUT_SHAPE, **R.WARP_LAYOUTS[label]))
  lay = R.WarpLayout(spec)
  B, nbg = R.LAYOUT_RAYS, (0 if lay.time else R.LAYOUT_BG)
  elastic = not lay.translation   # as tests/test_gpu_bf16_layouts.py: the elastic loss on for the SE3 fields
  p = O.init_params(spec, seed=5, trained_like=True, dtype=torch.float64)
  b = O.synthetic_batch(B, seed=6, dtype=torch.float64)
  g = torch.Generator().manual_seed(7)
  kw = dict(warp_alpha=R.ALPHA, t_rand=torch.rand(B, spec.num_coarse_samples, generator=g).double(),
            u=torch.rand(B, spec.num_fine_samples, generator=g).double())
  if lay.time:
    kw['time_alpha'] = R.LAYOUT_TIME_ALPHA
  if nbg:
    kw.update(use_background_loss=True, background_loss_weight=1.0,
              background={'points': (torch.rand(nbg, 3, generator=g).double() - 0.5) * 0.8, 'warp_ids': torch.randint(0, 4, (nbg,), generator=g),
                          'noise': 0.001 * torch.randn(nbg, 3, generator=g).double()})
  okw = dict(kw, use_elastic_loss=True, elastic_loss_weight=ELASTIC_WEIGHT, elastic_reduce_method='weight') if elastic else kw
  _, _, ograds, _ = O.loss_and_grad(p, spec, b, **okw)
  run = _oracle_run(spec, p, b, **kw)   # without the elastic term: it is added below on the recorded primal pass
  dense, act, total = run.dense, run.act, run.total
  wf = p['warp_field']
  weights = lay.weights(wf)
  XW, Win = lay.width, lay.Win
  S = (spec.num_coarse_samples, spec.num_coarse_samples + spec.num_fine_samples)
  heads = ['mlp/logit'] if lay.translation else ['branches_w/logit', 'branches_v/logit']
  tangents = None
  if elastic:
    X0 = dense[f'warp_field/{lay.trunk}/hidden_0'][0][0].detach().reshape(-1, Win)
    masks0 = [(act[('coarse/warp', l)][1].detach() > 0).reshape(-1, XW).double() for l in range(lay.depth)]
    wv0 = [dense[f'warp_field/{hn}'][0][1].reshape(-1, 3) for hn in heads]
    term, tangents = _tangent_pass(lay, spec, run, X0[:, :3], X0[:, 3 + 6 * lay.F:], masks0, wv0, run.ret['coarse']['weights'].detach())
    total = total + term
    # the hand-written forward-mode pass is the oracle's: every leaf of the whole tree, elastic term included
    for path, have, (_, ref) in zip(run.paths, _grad_of_unused(total, run.req), O.tree_leaves_with_path(ograds)):
      assert (have - ref).abs().max().item() <= TOL * max(ref.abs().max().item(), 1e-300), ('hand-written elastic pass', path)
  ray_ids = torch.arange(B) if lay.time else b['metadata']['warp'].reshape(-1).long()
  passes = [('coarse', ray_ids.repeat_interleave(S[0])), ('fine', ray_ids.repeat_interleave(S[1]))]
  if nbg:
    passes.append(('background', kw['background']['warp_ids'].long()))
  want, dcode_rows, dcode_ids = {}, [], []
  for i, (name, ids) in enumerate(passes):
    X = dense[f'warp_field/{lay.trunk}/hidden_0'][i][0].detach().reshape(-1, Win)
    pre = [act[(f'{name}/warp', l)][0] for l in range(lay.depth)]
    a = [act[(f'{name}/warp', l)][1] for l in range(lay.depth)]
    outs = [dense[f'warp_field/{hn}'][i][1] for hn in heads]
    grads = _grad_of(total, pre + [a[-1]] + outs)
    Hs = [t.detach().reshape(-1, XW) for t in a]
    DY = [t.reshape(-1, XW) for t in grads[:lay.depth]]
    for l in lay.identities:   # behind the caller's last layer: its activation again, and d activation under its own mask
      Hs.append(Hs[lay.depth - 1])
      DY.append(grads[lay.depth].reshape(-1, XW) * (Hs[lay.depth - 1] > 0))
    DH = torch.cat([t.reshape(-1, 3) for t in grads[lay.depth + 1:]], -1)
    if lay.translation:
      DH = torch.cat([torch.zeros_like(DH), DH], -1)
    masks = [t > 0 for t in Hs]
    r = R.warp_pass_from_stash(lay, weights, X, Hs, DY, DH, masks, False, R.exact)
    for l in range(R.WARP_DEPTH):   # the recomputed chain is the synthesised one
      assert (r['h'][l] - Hs[l]).abs().max().item() <= TOL * Hs[l].abs().max().item(), (name, 'h', l)
      assert (r['dpre'][l] - DY[l]).abs().max().item() <= TOL * max(DY[l].abs().max().item(), 1e-300), (name, 'dpre', l)
    assert (r['heads'][:, 3:] - outs[-1].detach().reshape(-1, 3)).abs().max().item() <= TOL
    R.add_leaves(want, r['leaves'])
    dcode_rows.append(r['dcode'])
    dcode_ids.append(ids)
    if i == 0:
      prim_masks = masks
  if elastic:   # the tangent pass: the three coordinates one behind the other, the primal coarse pass's ReLU pattern, no bias
    flat = [t for rec in tangents for t in rec['pre'] + [rec['h'][-1]] + rec['heads']]
    grads = _grad_of(total, flat)
    n = lay.depth + 3
    X = torch.cat([rec['X'] for rec in tangents], 0)
    Hs = [torch.cat([rec['h'][l].detach() for rec in tangents], 0) for l in range(lay.depth)]
    DY = [torch.cat([grads[c * n + l] for c in range(3)], 0) for l in range(lay.depth)]
    masks = [m.repeat(3, 1) for m in prim_masks]
    for l in lay.identities:
      Hs.append(Hs[lay.depth - 1])
      DY.append(torch.cat([grads[c * n + lay.depth] for c in range(3)], 0) * masks[lay.depth - 1])
    DH = torch.cat([torch.cat([grads[c * n + lay.depth + 1], grads[c * n + lay.depth + 2]], -1) for c in range(3)], 0)
    r = R.warp_pass_from_stash(lay, weights, X, Hs, DY, DH, masks, True, R.exact)
    for l in range(R.WARP_DEPTH):
      assert (r['h'][l] - Hs[l]).abs().max().item() <= TOL * Hs[l].abs().max().item(), ('tangent', 'h', l)
      assert (r['dpre'][l] - DY[l]).abs().max().item() <= TOL * max(DY[l].abs().max().item(), 1e-300), ('tangent', 'dpre', l)
    R.add_leaves(want, r['leaves'])
  time = b['metadata']['time'] if lay.time else None
  want.update(R.code_leaves(lay, wf, torch.cat(dcode_rows, 0), torch.cat(dcode_ids, 0), time, kw.get('time_alpha')))
  if lay.translation:   # the caller's tree is the TranslationField's: 'mlp', no 'trunk' / 'branches_*'
    assert 'mlp' in ograds['warp_field'] and not any(k.startswith('branches') or k == 'trunk' for k in ograds['warp_field'])
  errs = R.compare_leaves(want, ograds['warp_field'])
  bad = {k: v for k, v in errs.items() if not v < TOL}
  assert not bad, (label, bad)
  print(f'[{label}] identities {lay.identities}, tangent pass {elastic}: worst leaf {max(errs.values()):.1e}')
