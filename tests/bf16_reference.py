"""Same-rounding float64 references of the two bfloat16 training chains (csrc/mlp_bf16.hip + csrc/wgrad_bf16.hip, csrc/warp_bf16.hip),
for every model nrf_create lays out on them (csrc/nrf_api.hip nrf_create, csrc/nrf_plan.hip build_layout).

Everything here works GIVEN A STASH: the bfloat16 activations X and back-propagated pre-activation gradients dY of one pass, decoded to
float64 matrices.  Each stashed quantity is recomputed from the stashed quantity next to it with the roundings the kernels apply
(`q` = round to bfloat16: GEMM operands, every dpre before it is used; biases as a (hi, lo) pair; accumulation exact), and the
gradient leaves of the CALLER'S tree are X^T dY over the layers the caller owns.  The layout enters in three places only:

  * NeRF trunk: chain layer c (0..7) runs the caller's layer caller_of[c] or an internal identity (relu(h . I) = h for h >= 0); the
    chain's one skip GEMM sits at chain layer 4 and multiplies the posenc with the caller's skip layer's rows [tw:], or with zeros
    when the caller's trunk never reaches its skip (MlpLayout);
  * NeRF heads: without any condition there is no bottleneck leaf (an internal identity runs in its place); with
    use_alpha_condition the alpha head reads [bottleneck | appearance code] instead of the trunk output;
  * warp trunk: the caller's depth x width runs zero-padded on 6 x 128 with identities behind its last layer; the TranslationField's
    'mlp' leaves run as trunk + translation head with a rotation head that is identically zero (WarpLayout).

With q = the identity the same functions are the plain chain rule; tests/test_bf16_reference_host.py holds them against
oracle.loss_and_grad on a stash synthesised from the float64 oracle, so the layer maps, skip rows, missing bottleneck and leaf names
of THIS code are proven on the CPU before a kernel is compared with it.

What the time-encoded warp code rounds (csrc/time_encoder.hip, csrc/warp_bf16.hip): modules.TimeEncoder runs in float32 from end to
end -- posenc of the time stamp, six 64-wide layers, the output layer, its reverse pass and its weight gradients are float32 FMAs,
nothing is rounded to bfloat16.  Its (B, G) output takes the place of the GLO table with the ray number as the id: the trunk kernel
rounds a ray's code to bfloat16 exactly where it rounds a GLO row, as columns 3 + 6 F.. of the trunk input.  The code's gradient is
the code columns of dpre_0 . W0^T + dpre_4 . W4[W:]^T (bfloat16 operands, float32 accumulation) added per ray in float32; from
there the encoder's own chain rule is float32.  So the reference below takes the codes from a float64 evaluation of the encoder, and
differentiates that evaluation for the encoder's leaves given the stash's d code."""
import numpy as np
import torch

from oracle import nerfies_oracle as O
import helpers as H

DEV = H.DEV
SKIP = 4            # the chains' own skip layer (csrc/nrf_internal.h SKIP_LAYER / WARP_SKIP)
TRUNK_DEPTH = 8
WARP_DEPTH = 6
# the step-1 checks of the NeRF-MLP chain run the mode that keeps the SE3 trunk in float32 (NRF_FLAG_BF16 | NRF_FLAG_WARP_F32)
MLP = 'mlp'
WARP_ALPHA = 4.0    # tests/test_gpu_bf16_train.py
ALPHA = 4.3         # tests/test_gpu_bf16_warp.py


def exact(t):
  """the rounding function of the host test: none"""
  return t


def hilo(v, q):
  """biases and the alpha row ride as a (hi, lo) bfloat16 pair"""
  return q(v) + q(v - q(v))


# ---------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------
def close(got, want, what, atol_frac=2e-2, l2=5e-3, ulp_frac=0.05):
  """A stashed bfloat16 quantity against its recomputation.  One-ulp ties (float32 vs float64 accumulation, v_sin_f32 vs sin in the
  posenc) propagate: a unit near its kink may differ by a multiple of its own value, never by more than a few bfloat16 ulps of the
  layer's scale.  Largest deviation <= atol_frac x the layer's scale, relative L2 distance <= l2, fewer than ulp_frac of the elements
  off by more than one ulp.  Returns (max error / scale, relative L2, fraction)."""
  got, want = got.double(), want.double()
  scale = want.abs().max().item()
  err = (got - want).abs()
  assert err.max().item() <= atol_frac * scale + 1e-30, (what, err.max().item(), scale)
  if scale == 0:
    return 0.0, 0.0, 0.0
  rel = (err.norm() / want.norm()).item()
  assert rel <= l2, (what, rel)
  frac = (err > 2.0 ** -7 * want.abs() + 1e-6 * scale).double().mean().item()
  assert frac < ulp_frac, (what, frac)
  return err.max().item() / scale, rel, frac


def compare_leaves(want, tree, tw=None):
  """{path: |have - want|_max / |want|_max} of the leaves of `tree` (a nested dict of tensors) that `want` names.  A key 'path[:tw]' /
  'path[tw:]' is held against those rows of the leaf.  A leaf `tree` does not hold, a leaf of another shape, and a leaf of `tree`
  that `want` does not cover are assertion errors: the reference and the caller's tree name the same set of leaves."""
  errs, covered = {}, set()
  for key, w in want.items():
    path = key.replace('[:tw]', '').replace('[tw:]', '')
    try:
      have = H.leaf(tree, path).double()
    except KeyError:
      raise AssertionError(f'the reference computes {path}, which the tree does not hold')
    covered.add(path)
    if key.endswith('[:tw]'):
      have = have[:tw]
    elif key.endswith('[tw:]'):
      have = have[tw:]
    assert tuple(have.shape) == tuple(w.shape), (key, tuple(have.shape), tuple(w.shape))
    errs[key] = (have - w).abs().max().item() / max(w.abs().max().item(), 1e-30)
  left = [p for p, _ in O.tree_leaves_with_path(tree) if p not in covered]
  assert not left, f'leaves of the tree the reference has no value for: {left}'
  return errs


# ---------------------------------------------------------------------------------------------
# NeRF-MLP chain
# ---------------------------------------------------------------------------------------------
class MlpLayout:
  """How the caller's NeRF MLP lies on the 8-layer chain.  layer_map / skip_rows_at / bottleneck override what the spec implies: they
  exist for the negative controls of tests/test_bf16_reference_host.py."""

  def __init__(self, spec, layer_map=None, skip_rows_at=None, bottleneck=None):
    self.depth = spec.nerf_trunk_depth
    self.skip = spec.nerf_skips[0] if (len(spec.nerf_skips) and spec.nerf_skips[0] < self.depth) else -1
    self.chain_of = list(H.trunk_layer_map(spec)[:self.depth] if layer_map is None else layer_map)   # caller's layer -> chain layer
    self.caller_of = [-1] * TRUNK_DEPTH                                                              # chain layer -> caller's, -1 = identity
    for e, c in enumerate(self.chain_of):
      self.caller_of[c] = e
    self.identities = [c for c in range(TRUNK_DEPTH) if self.caller_of[c] < 0]
    self.skip_rows_at = self.skip if skip_rows_at is None else skip_rows_at     # the caller's layer whose kernel holds posenc rows
    self.tw, self.rw, self.P = spec.nerf_trunk_width, spec.nerf_rgb_branch_width, 3 + 6 * spec.num_nerf_point_freqs
    self.A = spec.alpha_cond_width                                              # > 0: the alpha head reads [bottleneck | code]
    self.bottleneck = (spec.rgb_cond_width > 0 or self.A > 0) if bottleneck is None else bottleneck


def bf16_dense_for(spec, params):
  """csrc/mlp_bf16.hip's arithmetic of one Dense of the NeRF MLPs of `params` (the tree the oracle is evaluated on), as an
  oracle.dense_hook: bf16 operands, exact bias, dY rounded.  Two layers are told by the identity of their parameter dict, not by
  their shape: the rgb hidden layer rounds only the bottleneck rows (the per-ray condition columns are folded into an exact float32
  term by ray_prep), and the alpha head under use_alpha_condition rounds only its bottleneck rows (the appearance-code rows are a
  float32 per-ray term as well).  (The forward stream holds the alpha head's weights as single bfloat16 values; the (hi, lo) pair is
  the reverse stream's, mlp_leaves_from_stash.)"""
  tw = spec.nerf_trunk_width
  rgb_hidden = {id(params[k]['MLP_1']['hidden_0']) for k in ('nerf_mlps_coarse', 'nerf_mlps_fine') if k in params}
  alpha_head = {id(params[k]['MLP_2']['logit']) for k in ('nerf_mlps_coarse', 'nerf_mlps_fine') if k in params}

  def dense(p, x):
    w = p['kernel']
    if O._SCOPE != 'nerf_mlp':   # the warp field stays float32 in this mode
      return x @ w + p['bias']
    nq = tw if (id(p) in rgb_hidden or id(p) in alpha_head) else w.shape[0]
    y = _RoundFwd.apply(x[..., :nq]) @ _RoundFwd.apply(w[:nq])
    if nq < w.shape[0]:
      y = y + x[..., nq:] @ w[nq:]
    return _RoundBwd.apply(y + p['bias'])
  return dense


class _RoundFwd(torch.autograd.Function):
  """x -> bfloat16(x) (RNE), gradient passed through (the master copy is float32)."""

  @staticmethod
  def forward(ctx, x):
    return x.to(torch.bfloat16).to(x.dtype)

  @staticmethod
  def backward(ctx, g):
    return g


class _RoundBwd(torch.autograd.Function):
  """identity whose incoming gradient is rounded to bfloat16 (the dY stash)."""

  @staticmethod
  def forward(ctx, x):
    return x.view_as(x)

  @staticmethod
  def backward(ctx, g):
    return g.to(torch.bfloat16).to(g.dtype)


def mlp_leaves_from_stash(lay, prm, st, q, code=None, dsig_ray=None):
  """One level's dgrad chain and weight gradients from its forward stash.

  prm: the level's parameters in the CALLER'S naming (float64).  st: dict(pe (rows, P), h [8 x (rows, tw)] in CHAIN order, bn
  (rows, tw), rgbh (rows, rw), draw (rows, 4) = d raw rgb, d raw sigma).  code (B, A) / dsig_ray (B, 1): under use_alpha_condition
  the per-ray appearance code and the per-ray sum of d raw sigma (its term of the alpha head is a float32 per-ray scalar).
  Returns (want, aux): want = {caller's leaf path: gradient}, aux = dict(dpre {chain layer: (rows, tw)}, drgbh, dbn, dpe (rows, P))."""
  tw, P = lay.tw, lay.P
  pe, h, bn, rgbh, draw = st['pe'], st['h'], st['bn'], st['rgbh'], st['draw']

  def W(path):
    try:
      return H.leaf(prm, path)
    except KeyError:
      raise AssertionError(f'the reference reads {path}, which the tree does not hold')
  dlog, dsig = draw[:, :3], draw[:, 3:4]
  want = {}
  want['MLP_1/logit/kernel'], want['MLP_1/logit/bias'] = rgbh.T @ dlog, dlog.sum(0)
  drgbh = q((dlog @ q(W('MLP_1/logit/kernel')).T) * (rgbh > 0))
  want['MLP_1/hidden_0/kernel[:tw]'], want['MLP_1/hidden_0/bias'] = bn.T @ drgbh, drgbh.sum(0)
  wa = hilo(W('MLP_2/logit/kernel')[:tw], q)
  d = drgbh @ q(W('MLP_1/hidden_0/kernel')[:tw]).T
  if lay.A:    # the alpha head reads the bottleneck: its row joins d bottleneck, its code rows are a per-ray product
    d = d + dsig @ wa.T
    want['MLP_2/logit/kernel[:tw]'] = bn.T @ dsig
    want['MLP_2/logit/kernel[tw:]'] = code.T @ dsig_ray
  else:
    want['MLP_2/logit/kernel'] = h[7].T @ dsig
  want['MLP_2/logit/bias'] = dsig.sum(0)
  dbn = q(d)
  if lay.bottleneck:
    want['bottleneck/kernel'], want['bottleneck/bias'] = h[7].T @ dbn, dbn.sum(0)
    d = dbn @ q(W('bottleneck/kernel')).T
  else:        # the internal identity: d h8 = d bottleneck, no leaf
    d = dbn
  if not lay.A:
    d = d + dsig @ wa.T
  d = q(d * (h[7] > 0))
  dpre, dpe = {}, 0.0
  eye = torch.eye(tw, dtype=pe.dtype)
  for c in range(TRUNK_DEPTH - 1, -1, -1):
    dpre[c] = d
    e = lay.caller_of[c]
    x = h[c - 1] if c > 0 else pe
    if e >= 0:
      wk = W(f'MLP_0/hidden_{e}/kernel')
      gk = x.T @ d
      if e > 0 and e == lay.skip_rows_at:   # the layer that reads [h, posenc] (modules.py:47-48)
        assert wk.shape[0] == tw + P, f'the reference takes posenc rows from MLP_0/hidden_{e}, whose kernel has {wk.shape[0]} rows'
        gk = torch.cat([gk, pe.T @ d], 0)
        dpe = dpe + d @ q(wk[tw:]).T
      want[f'MLP_0/hidden_{e}/kernel'], want[f'MLP_0/hidden_{e}/bias'] = gk, d.sum(0)
      wmain = wk[:tw] if c > 0 else wk
    else:      # identity layer: relu(h . I + 0), nothing of it reaches the caller's tree
      wmain = eye
    if c > 0:
      d = q((d @ q(wmain).T) * (h[c - 1] > 0))
    else:
      dpe = dpe + d @ q(wmain).T
  return want, dict(dpre=dpre, drgbh=drgbh, dbn=dbn, dpe=dpe)


def mlp_setup(B, seed=3, **kw):
  spec = O.ModelSpec(**dict(dict(num_coarse_samples=64, num_fine_samples=128, num_nerf_point_freqs=8, use_stratified_sampling=True), **kw))
  p = O.init_params(spec, seed=seed, trained_like=True, dtype=torch.float64)
  b = O.synthetic_batch(B, seed=seed + 1, dtype=torch.float64)
  g = torch.Generator().manual_seed(seed + 2)
  t_rand = torch.rand(B, spec.num_coarse_samples, generator=g).double()
  u = torch.rand(B, spec.num_fine_samples, generator=g).double()
  model, fp = H.gpu_model(spec, p, B)
  rngs = {'coarse': t_rand.float().to(DEV), 'fine': u.float().to(DEV)}
  return spec, p, b, t_rand, u, model, fp, rngs


def _levels(spec, B):
  S = (spec.num_coarse_samples, spec.num_coarse_samples + spec.num_fine_samples)
  return [(lv, name, B * S[lv]) for lv, name in enumerate(('coarse', 'fine') if spec.num_fine_samples > 0 else ('coarse',))]


def check_forward_and_stash(setup, ulp_frac=0.05):
  """Step 1a: loss, rendered outputs and every stashed activation against the float64 oracle with the same roundings.
  float32 vs float64 accumulation moves a pre-activation by ~1e-7 relative, which flips the bfloat16 rounding of about
  one element in 3000 by one ulp (0.4 %), and later layers inherit those: per layer the relative L2 distance stays below
  5e-3, the largest deviation below 2 % of the layer's scale, at least 95 % of the elements within one ulp.

  The caller's layer e is found at chain layer chain_of[e]; an identity layer's stash equals the stash in front of it bit for bit,
  the internal identity of a model without a bottleneck leaves the trunk output in the bottleneck's stash, and the padded units of a
  narrower trunk / rgb branch are zero.  Returns the worst (max error / scale) over the compared activations."""
  spec, p, b, t_rand, u, model, fp, rngs = setup
  lay = MlpLayout(spec)
  B = b['origins'].shape[0]
  gb = H.gpu_batch(b)
  grad, stats = model.loss_and_grad(fp, gb, warp_extra={'alpha': WARP_ALPHA}, rngs=rngs, bf16=MLP)
  torch.cuda.synchronize()
  ws = model.workspace(B, True, DEV, bf16=MLP)
  S1 = spec.num_coarse_samples + spec.num_fine_samples
  fine = spec.num_fine_samples > 0
  z_fine = torch.from_numpy(H._ws_words(model, ws, 'z', 1, B * S1).view('float32').reshape(B, S1).copy()).double() if fine else None
  acts = {}

  def record(name, layer, pre):
    acts[(name, layer)] = H.bf16_round(torch.relu(pre.detach())).float()   # exact in float32, half the host memory
    return torch.relu(pre)
  with H.host_threads(64), torch.no_grad(), O.dense_hook(bf16_dense_for(spec, p)), O.relu_hook(record):   # forward only: no graph
    loss, ostats, ret = O.loss_fn(p, spec, b, warp_alpha=WARP_ALPHA, t_rand=t_rand, u=u, fixed_fine_z=z_fine)
  assert abs(stats[4].item() - loss.item()) < 5e-5, (stats[4].item(), loss.item())
  tw, rw = lay.tw, lay.rw
  worst = 0.0
  for lv, name, rows in _levels(spec, B):
    hs = H.bf16_stash(model, ws, 'b_h', lv, 8, 8, rows, as_float32=True)
    rg = H.bf16_stash(model, ws, 'b_rgbh', lv, 1, 4, rows, as_float32=True)[0]
    for e, c in enumerate(lay.chain_of):
      worst = max(worst, close(hs[c][:, :tw], acts[(f'{name}/MLP_0', e)], (name, e, c), ulp_frac=ulp_frac)[0])
    for c in range(TRUNK_DEPTH):
      assert (hs[c][:, tw:] == 0).all(), (name, c)   # padded units of a narrower trunk stay dead
    for c in lay.identities:
      assert torch.equal(hs[c], hs[c - 1]), (name, 'identity layer', c)
    worst = max(worst, close(rg[:, :rw], acts[(f'{name}/MLP_1', 0)], (name, 'rgb hidden'), ulp_frac=ulp_frac)[0])
    assert (rg[:, rw:] == 0).all(), (name, 'rgb hidden padding')
    if not lay.bottleneck:
      bn = H.bf16_stash(model, ws, 'b_bn', lv, 1, 8, rows, as_float32=True)[0]
      assert torch.equal(bn, hs[7]), (name, 'bottleneck identity')
  out = model.apply({'params': fp}, gb, {'alpha': WARP_ALPHA}, rngs=rngs, return_weights=True, bf16=MLP)
  for lv in out:
    np.testing.assert_allclose(out[lv]['weights'].cpu().numpy(), ret[lv]['weights'].detach().numpy(), atol=1e-4)
    np.testing.assert_allclose(out[lv]['rgb'].cpu().numpy(), ret[lv]['rgb'].detach().numpy(), atol=1e-3)
  return worst


def check_backward_given_the_stash(setup, report=None):
  """Step 1b: the dgrad chain and the transposing wgrad kernel against a float64 evaluation of the SAME quantities from
  the kernels' own forward stash (bfloat16 activations X, bfloat16 d raw, bfloat16 weights, every dpre rounded to
  bfloat16 before use): all weight / bias gradient leaves to 5e-3 of the leaf's max-abs (measured 5e-5 .. 2e-3: a dpre within
  float32 rounding of a bfloat16 tie rounds the other way in float64, and at a few thousand rows one such element shows).  (The end-to-end comparison with
  the rounded oracle is not used for the gradients: the one-ulp rounding ties of step 1a, harmless in the rendered
  colour, are amplified by the cancellation inside d sigma = T (c_i - C_behind) to percents of the density gradient.)

  Where the layout has identity layers (or the internal bottleneck), their stashed dpre is checked as well: equal to the stashed
  dpre behind it bit for bit when that is an identity too, else its recomputation from the stash behind it within the activation
  bounds; and every NeRF-MLP leaf of the caller's tree is covered by the reference, so nothing of an identity can sit in one.
  Returns the flat gradient; report['worst_leaf'] = (leaf, its error) if a dict is given."""
  from nerfies_amd import params as P
  spec, p, b, t_rand, u, model, fp, rngs = setup
  lay = MlpLayout(spec)
  B = b['origins'].shape[0]
  grad, stats = model.loss_and_grad(fp, H.gpu_batch(b), warp_extra={'alpha': WARP_ALPHA}, rngs=rngs, bf16=MLP)
  torch.cuda.synchronize()
  ws = model.workspace(B, True, DEV, bf16=MLP)
  got = P.tree_from_flat(grad.cpu(), model.layout)
  tw, rw, P_ = lay.tw, lay.rw, lay.P
  q = H.bf16_round
  worst = ('', 0.0)
  for lv, lname, rows in _levels(spec, B):
    name = f'nerf_mlps_{lname}'
    prm = O.tree_map(lambda t: t.float().double(), p[name])     # the float32 master weights
    st = dict(pe=H.bf16_stash(model, ws, 'b_pe', lv, 1, 2, rows)[0][:, :P_],
              h=[t[:, :tw] for t in H.bf16_stash(model, ws, 'b_h', lv, 8, 8, rows)],
              bn=H.bf16_stash(model, ws, 'b_bn', lv, 1, 8, rows)[0][:, :tw],
              rgbh=H.bf16_stash(model, ws, 'b_rgbh', lv, 1, 4, rows)[0][:, :rw],
              draw=H.bf16_stash(model, ws, 'b_dsmall', lv, 1, 2, rows)[0][:, :4])
    code = dsig_ray = None
    if lay.A:
      code = p['appearance_encoder']['embed']['embedding'][b['metadata']['appearance'][:, 0].long()].float().double()
      d4 = torch.from_numpy(H._ws_words(model, ws, 'd_raw4', lv, rows * 4).view('float32').reshape(B, rows // B, 4).copy()).double()
      dsig_ray = d4[..., 3].sum(1, keepdim=True)
    want, aux = mlp_leaves_from_stash(lay, prm, st, q, code, dsig_ray)
    if lay.identities or not lay.bottleneck or tw < 256 or rw < 128:
      dy = H.bf16_stash(model, ws, 'b_dy', lv, 8, 8, rows)
      dbn = H.bf16_stash(model, ws, 'b_dbn', lv, 1, 8, rows)[0]
      drg = H.bf16_stash(model, ws, 'b_drgbh', lv, 1, 4, rows)[0]
      for c in range(TRUNK_DEPTH):   # a padded unit is dead in the reverse chain too
        assert (dy[c][:, tw:] == 0).all(), (name, 'dpre of the padded units', c)
      assert (dbn[:, tw:] == 0).all() and (drg[:, rw:] == 0).all(), (name, 'd bottleneck / d rgb hidden of the padded units')
      dy, dbn = [t[:, :tw] for t in dy], dbn[:, :tw]
      if not lay.bottleneck or TRUNK_DEPTH - 1 in lay.identities:   # dpre_7 from the stashed d bottleneck behind it
        d = dbn @ q(H.leaf(prm, 'bottleneck/kernel')).T if lay.bottleneck else dbn
        if not lay.A:
          d = d + st['draw'][:, 3:4] @ hilo(H.leaf(prm, 'MLP_2/logit/kernel')[:tw], q).T
        close(dy[7], q(d * (st['h'][7] > 0)), (name, 'dpre_7 from the stashed d bottleneck'))
      for c in lay.identities:
        if c == TRUNK_DEPTH - 1:
          pass   # (above)
        elif c + 1 in lay.identities:
          assert torch.equal(dy[c], dy[c + 1]), (name, 'dpre of identity layer', c)
        else:
          wk = H.leaf(prm, f'MLP_0/hidden_{lay.caller_of[c + 1]}/kernel')[:tw]
          close(dy[c], q((dy[c + 1] @ q(wk).T) * (st['h'][c] > 0)), (name, 'dpre of identity layer', c))
    for path, err in compare_leaves(want, {k: v for k, v in got[name].items()}, tw).items():
      worst = max(worst, (f'{name}/{path}', err), key=lambda t: t[1])
      assert err < 5e-3, (name, path, err)
    if spec.use_warp:   # d points = chain rule of the posenc applied to d posenc = dpre_0 . W0^T + dpre_skip . W_skip[tw:]^T
      rows_pad = (rows + 63) // 64 * 64
      x = torch.from_numpy(H._ws_words(model, ws, 'wpoints', lv, rows_pad * 3).view('float32').reshape(rows_pad, 3)[:rows].copy()).double()
      have = torch.from_numpy(H._ws_words(model, ws, 'd_points', lv, rows_pad * 3).view('float32').reshape(rows_pad, 3)[:rows].copy()).double()
      dpe = aux['dpe']
      dx = dpe[:, :3].clone()
      for f in range(spec.num_nerf_point_freqs):
        a = (x.float() * float(2 ** f)).double()
        dx += 2.0 ** f * (torch.cos(a) * dpe[:, 3 + 6 * f:6 + 6 * f] - torch.sin(a) * dpe[:, 6 + 6 * f:9 + 6 * f])
      err = (have - dx).abs().max().item() / dx.abs().max().item()
      worst = max(worst, (f'{name}/d_points', err), key=lambda t: t[1])
      assert err < 5e-3, (name, 'd_points', err)
  print(f'[bf16 backward given the stash, B={B}] worst leaf {worst[0]}: {worst[1]:.2e}')
  if report is not None:
    report['worst_leaf'] = worst
  return grad


def check_inference_matches_training(setup):
  """bf16 inference (no stash) renders what the training forward renders (tests/test_gpu_bf16.py: 1e-6 on the default layout)."""
  spec, p, b, t_rand, u, model, fp, rngs = setup
  gb = H.gpu_batch(b)
  tr = model.apply({'params': fp}, gb, {'alpha': WARP_ALPHA}, rngs=rngs, train=True, bf16=MLP)
  tr = {lv: tr[lv]['rgb'].clone() for lv in tr}
  inf = model.apply({'params': fp}, gb, {'alpha': WARP_ALPHA}, rngs=rngs, bf16=MLP)
  for lv in tr:
    np.testing.assert_allclose(tr[lv].cpu().numpy(), inf[lv]['rgb'].cpu().numpy(), atol=1e-6)


# ---------------------------------------------------------------------------------------------
# warp trunk
# ---------------------------------------------------------------------------------------------
class WarpLayout:
  """How the caller's warp field lies on the 6 x 128 trunk: depth x width, SE3Field or TranslationField, GLO table or TimeEncoder."""

  def __init__(self, spec):
    self.depth, self.width = spec.warp_trunk_depth, spec.warp_trunk_width
    self.translation = spec.warp_field_type == 'translation'
    self.time = spec.warp_metadata_encoder_type == 'time'
    self.F, self.G, self.Ft = spec.num_warp_freqs, spec.num_warp_features, spec.num_time_encoder_freqs
    self.Win = 3 + 6 * self.F + self.G
    self.trunk = 'mlp' if self.translation else 'trunk'
    self.identities = list(range(self.depth, WARP_DEPTH))

  def weights(self, wf):
    """(Wk, bk, Wh, bh) of the six chain layers and the (w, v) heads at the caller's width, from the caller's float64 tree `wf`:
    identity layers behind the caller's last one (zero posenc rows at layer 4), a zero rotation head for the TranslationField."""
    XW, Win = self.width, self.Win
    some = wf[self.trunk]['hidden_0']['kernel']
    Wk, bk = [], []
    for l in range(WARP_DEPTH):
      if l < self.depth:
        Wk.append(wf[self.trunk][f'hidden_{l}']['kernel'])
        bk.append(wf[self.trunk][f'hidden_{l}']['bias'])
      else:
        eye = torch.eye(XW, dtype=some.dtype)
        Wk.append(torch.cat([eye, torch.zeros(Win, XW, dtype=some.dtype)], 0) if l == SKIP else eye)
        bk.append(torch.zeros(XW, dtype=some.dtype))
    if self.translation:
      Wh = torch.cat([torch.zeros(XW, 3, dtype=some.dtype), wf['mlp']['logit']['kernel']], 1)
      bh = torch.cat([torch.zeros(3, dtype=some.dtype), wf['mlp']['logit']['bias']])
    else:
      Wh = torch.cat([wf['branches_w']['logit']['kernel'], wf['branches_v']['logit']['kernel']], 1)
      bh = torch.cat([wf['branches_w']['logit']['bias'], wf['branches_v']['logit']['bias']])
    return Wk, bk, Wh, bh


def warp_pass_from_stash(lay, weights, X, Hs, DY, DH, masks, tangent, q):
  """One pass through the field (the samples of a level, the background points, or the three tangents per coarse sample), every stage
  from the stashed stage in front of it.  X (rows, Win) trunk input, Hs / DY [6 x (rows, XW)] activations / dpre, DH (rows, 6) d
  (w, v), masks [6 x bool (rows, XW)] the PRIMAL pass's ReLU pattern.  Returns dict(h [6] recomputed activations, heads (rows, 6),
  dpre {l: recomputed}, leaves {caller's path: this pass's contribution}, dcode (rows, G))."""
  Wk, bk, Wh, bh = weights
  XW, Win = lay.width, lay.Win
  out = dict(h=[], dpre={}, leaves={})
  for l in range(WARP_DEPTH):
    Wl = Wk[l]
    if l == 0:
      pre = X @ q(Wl)
    elif l == SKIP:
      pre = Hs[l - 1] @ q(Wl[:XW]) + X @ q(Wl[XW:])
    else:
      pre = Hs[l - 1] @ q(Wl)
    out['h'].append(q(pre * masks[l]) if tangent else q(torch.relu(pre + hilo(bk[l], q))))
  out['heads'] = Hs[5] @ q(Wh) + (0 if tangent else hilo(bh, q))
  out['dpre'][5] = q((DH[:, :6] @ q(Wh).T) * masks[5])
  for l in range(5, 0, -1):
    out['dpre'][l - 1] = q((DY[l] @ q(Wk[l][:XW]).T) * masks[l - 1])
  # the leaves' gradients: X^T dY over the rows of this pass (tangent: no bias, training.py / warping.py:385-387)
  lv = out['leaves']
  for l in range(lay.depth):
    gk = (X if l == 0 else Hs[l - 1]).T @ DY[l]
    if l == SKIP:
      gk = torch.cat([gk, X.T @ DY[l]], 0)
    lv[f'{lay.trunk}/hidden_{l}/kernel'] = gk
    if not tangent:
      lv[f'{lay.trunk}/hidden_{l}/bias'] = DY[l].sum(0)
  heads = (('mlp/logit', 3),) if lay.translation else (('branches_w/logit', 0), ('branches_v/logit', 3))
  for hn, c0 in heads:
    lv[f'{hn}/kernel'] = Hs[5].T @ DH[:, c0:c0 + 3]
    if not tangent:
      lv[f'{hn}/bias'] = DH[:, c0:c0 + 3].sum(0)
  out['dcode'] = (DY[0] @ q(Wk[0]).T + DY[SKIP] @ q(Wk[SKIP][XW:]).T)[:, 3 + 6 * lay.F:Win]
  return out


def code_leaves(lay, wf, dcode_rows, ids, time=None, time_alpha=None):
  """The metadata encoder's leaves from d code per row: the GLO table's rows summed per id, or (TimeEncoder) the float64 chain rule of
  the encoder applied to the per-ray sums."""
  if not lay.time:
    table = wf['metadata_encoder']['embed']['embedding']
    return {'metadata_encoder/embed/embedding': torch.zeros_like(table).index_add_(0, ids, dcode_rows)}
  enc = wf['metadata_encoder']
  leaves = list(O.tree_leaves_with_path(enc))
  req = [t.detach().clone().requires_grad_(True) for _, t in leaves]
  it = iter(req)
  codes = O.time_encode(O.tree_map(lambda _: next(it), enc), time, lay.Ft, time_alpha)
  dcodes = torch.zeros_like(codes).index_add_(0, ids, dcode_rows)
  grads = torch.autograd.grad((codes * dcodes).sum(), req, allow_unused=True)
  return {f'metadata_encoder/{path}': (g if g is not None else torch.zeros_like(t)) for (path, t), g in zip(leaves, grads)}


def add_leaves(total, part):
  for k, v in part.items():
    total[k] = total[k] + v if k in total else v
  return total


def warp_setup(B, seed=5, nbg=0, head_scale=1.0, **kw):
  spec = O.ModelSpec(**dict(dict(num_coarse_samples=32, num_fine_samples=32, num_nerf_point_freqs=8, use_stratified_sampling=True,
                                 use_warp=True, num_warp_freqs=8, num_warp_features=8), **kw))
  p = O.init_params(spec, seed=seed, trained_like=True, dtype=torch.float64)
  if head_scale != 1.0:   # the "trained-like" heads throw points several scene sizes away; a capture's deformations are ~ 0.05
    heads = [p['warp_field']['mlp']] if spec.warp_field_type == 'translation' else [p['warp_field'][br] for br in ('branches_w', 'branches_v')]
    for hd in heads:
      for k in ('kernel', 'bias'):
        hd['logit'][k] = hd['logit'][k] * head_scale
  b = O.synthetic_batch(B, seed=seed + 1, dtype=torch.float64)
  g = torch.Generator().manual_seed(seed + 2)
  rngs = {'coarse': torch.rand(B, spec.num_coarse_samples, generator=g).to(DEV),
          'fine': torch.rand(B, spec.num_fine_samples, generator=g).to(DEV)}
  model, fp = H.gpu_model(spec, p, B)
  bg = None
  if nbg:
    bg = {'points': ((torch.rand(nbg, 3, generator=g) - 0.5) * 0.8).to(DEV), 'warp_ids': torch.randint(0, 4, (nbg,), generator=g).to(DEV),
          'weight': 1.0}
  return spec, p, b, model, fp, rngs, bg


def _f32rows(model, ws, name, lv, rows, width):
  return torch.from_numpy(H._ws_words(model, ws, name, lv, rows * width).view('float32').reshape(rows, width).copy()).double()


def _window(alpha, F):
  k = torch.arange(F, dtype=torch.float64)
  return 0.5 * (1 + torch.cos(np.pi * torch.clip(torch.tensor(alpha, dtype=torch.float64) - k, 0, 1) + np.pi))


def trunk_input(x, code, alpha, F, tangent_dir=None):
  """[annealed posenc(x), code] (warping.py:326-327, modules.py:231-294) or its derivative along one coordinate."""
  w = _window(alpha, F)
  cols = []
  if tangent_dir is None:
    cols.append(x)
    for f in range(F):
      a = (x.float() * float(2 ** f)).double()
      cols += [w[f] * torch.sin(a), w[f] * torch.sin((a.float() + np.float32(np.pi / 2)).double())]
    cols.append(code)
  else:
    e = torch.zeros_like(x); e[:, tangent_dir] = 1
    cols.append(e)
    for f in range(F):
      a = (x.float() * float(2 ** f)).double()
      cols += [w[f] * 2.0 ** f * torch.cos(a) * e, -w[f] * 2.0 ** f * torch.sin(a) * e]
    cols.append(torch.zeros_like(code))
  return torch.cat(cols, -1)


def check_warp_given_the_stash(setup, nbg, elastic=True, time_alpha=None):
  """Every stashed quantity of every pass through the bfloat16 warp trunk (coarse / fine samples, background points, with `elastic`
  the three tangents per coarse sample) from the stashed quantity in front of it, and the warp field's gradient leaves from the
  (X, dY) stashes summed over the passes: activations within the bounds of `close`, leaves to 5e-3 of the leaf's max-abs.  Exact:
  the padded units of a narrower trunk (activations and dpre zero), identity layers behind the caller's last one (stash equal to
  the stash in front of it), padding rows without gradient, the TranslationField's rotation head (w = 0 on every row).
  Returns (worst activation max error / scale, (worst leaf, its error))."""
  from nerfies_amd import params as P
  spec, p, b, model, fp, rngs, bg = setup
  lay = WarpLayout(spec)
  q = H.bf16_round
  B = b['origins'].shape[0]
  F, XW, Win = lay.F, lay.width, lay.Win
  gb = H.gpu_batch(b)
  wextra = {'alpha': ALPHA} if time_alpha is None else {'alpha': ALPHA, 'time_alpha': time_alpha}
  extra = dict(elastic={'weight': 0.01, 'reduce_method': 'weight'}) if elastic else {}
  grad, stats = model.loss_and_grad(fp, gb, warp_extra=wextra, rngs=rngs, bf16=True, background=bg, **extra)
  torch.cuda.synchronize()
  assert torch.isfinite(grad).all() and torch.isfinite(stats).all()
  ws = model.workspace(B, True, DEV, nbg, elastic, bf16=True)
  got = P.tree_from_flat(grad.cpu(), model.layout)['warp_field']
  wf = O.tree_map(lambda t: t.float().double(), p['warp_field'])
  weights = lay.weights(wf)
  if lay.time:
    time = b['metadata']['time'].float().double()
    with torch.no_grad():
      table = O.time_encode(wf['metadata_encoder'], time, lay.Ft, time_alpha)   # (B, G): a table indexed by the ray number
    ray_ids = torch.arange(B)
  else:
    time = None
    table = wf['metadata_encoder']['embed']['embedding']
    ray_ids = b['metadata']['warp'].reshape(-1).long()
  S = (spec.num_coarse_samples, spec.num_coarse_samples + spec.num_fine_samples)
  want, dcode_rows, dcode_ids = {}, [], []
  worst_act = 0.0
  passes = [('coarse', 0, B * S[0], False), ('fine', 1, B * S[1], False)]
  if nbg:
    passes.append(('background', 2, nbg, False))
  if elastic:
    passes.append(('tangent', 3, B * S[0], True))
  # (pass name, level in the workspace, rows, tangent?)
  for name, lv, rows, tangent in passes:
    ngp = (rows + 255) // 256 * 8                      # groups of the (primal) level
    ng = 3 * ngp if tangent else ngp
    nrow = ng * 32
    X = H.bf16_stash(model, ws, 'bw_in', lv, 1, 2, nrow, ngroups=ng)[0]
    Hs = H.bf16_stash(model, ws, 'bw_h', lv, 6, 4, nrow, ngroups=ng)
    DY = H.bf16_stash(model, ws, 'bw_dy', lv, 6, 4, nrow, ngroups=ng)
    DH = H.bf16_stash(model, ws, 'bw_dhead', lv, 1, 2, nrow, ngroups=ng)[0]
    valid = torch.zeros(nrow, dtype=torch.bool)
    if tangent:
      for c in range(3):
        valid[c * ngp * 32:c * ngp * 32 + rows] = True
    else:
      valid[:rows] = True
    for l in range(WARP_DEPTH):   # padded units of a narrower trunk stay dead, forward and backward
      assert (Hs[l][:, XW:] == 0).all() and (DY[l][:, XW:] == 0).all(), (name, 'padded units', l)
    assert (X[:, Win:] == 0).all()
    Hs, DY = [t[:, :XW] for t in Hs], [t[:, :XW] for t in DY]
    # ---- forward chain, each stage from the stashed stage in front of it ----
    if not tangent:
      rows_pad = (rows + 63) // 64 * 64
      if lv == 2:
        x = bg['points'].cpu().double()
        ids = bg['warp_ids'].cpu().long()
      else:
        x = _f32rows(model, ws, 'points_raw', lv, rows_pad, 3)[:rows]
        ids = ray_ids.repeat_interleave(S[lv])
      want_in = trunk_input(x, table[ids], ALPHA, F)
      close(X[:rows, :Win], q(want_in), (name, 'trunk input'), ulp_frac=0.02)
      masks = [(Hs[l] > 0) for l in range(6)]
      if lv == 0:
        prim_x, prim_ids, prim_masks = x, ids, masks
      wv = _f32rows(model, ws, 'w_st_wv', lv, rows_pad, 8)[:rows]
    else:
      masks = [m[:ngp * 32].repeat(3, 1) for m in prim_masks]
      for c in range(3):
        want_in = trunk_input(prim_x, table[prim_ids], ALPHA, F, tangent_dir=c)
        close(X[c * ngp * 32:c * ngp * 32 + rows, :Win], q(want_in), (name, 'tangent input', c), ulp_frac=0.02)
      wv = _f32rows(model, ws, 'w_st_wv', lv, 3 * ((rows + 63) // 64 * 64), 8)
      rp = (rows + 63) // 64 * 64
      wv = torch.cat([wv[c * rp:c * rp + rows] for c in range(3)], 0)
    r = warp_pass_from_stash(lay, weights, X[:, :Win], Hs, DY, DH, masks, tangent, q)
    for l in range(WARP_DEPTH):
      worst_act = max(worst_act, close(Hs[l][valid], r['h'][l][valid], (name, f'h{l + 1}'))[0])
    for l in lay.identities:
      assert torch.equal(Hs[l][valid], Hs[l - 1][valid]), (name, 'identity layer', l)
    hv = valid.nonzero().reshape(-1)
    heads = r['heads']
    got_wv = torch.cat([wv[:, 0:3], wv[:, 4:7]], 1)
    np.testing.assert_allclose(got_wv.numpy(), heads[hv].numpy(), atol=2e-5 * max(heads.abs().max().item(), 1e-3) + 1e-7, err_msg=f'{name} heads')
    if lay.translation:
      assert (wv[:, 0:3] == 0).all(), (name, 'the rotation head of a TranslationField')
    # ---- reverse chain ----
    for l in range(5, -1, -1):
      worst_act = max(worst_act, close(DY[l][valid], r['dpre'][l][valid], (name, f'dpre_{l}'))[0])
    assert (DY[0][~valid] == 0).all() and (DH[~valid] == 0).all()      # padding rows carry no gradient
    add_leaves(want, r['leaves'])
    if not tangent:   # (the tangent input does not depend on the code)
      dcode_rows.append(r['dcode'][:rows])
      dcode_ids.append(ids)
  # the code's gradient: d code = the code columns of (dpre_0 . W0^T + dpre_4 . W4[W:]^T), summed per warp id (per ray: TimeEncoder)
  # over the primal passes
  want.update(code_leaves(lay, wf, torch.cat(dcode_rows, 0), torch.cat(dcode_ids, 0), time, time_alpha))
  worst = ('', 0.0)
  for path, err in compare_leaves(want, got).items():
    worst = max(worst, (path, err), key=lambda t: t[1])
    assert err < 5e-3, (path, err)
  print(f'[bf16 warp trunk given the stash, {lay.depth} x {XW} {spec.warp_field_type} {spec.warp_metadata_encoder_type}, B={B}] worst activation '
        f'{worst_act:.2e}, worst leaf {worst[0]}: {worst[1]:.2e}')
  return worst_act, worst


# ---------------------------------------------------------------------------------------------
# The layouts of tests/test_bf16_reference_host.py (CPU: the references against oracle.loss_and_grad) and
# tests/test_gpu_bf16_layouts.py (the kernels against the references).  5 rays of 8 coarse + 6 fine samples are 40 and 70 rows: the
# second 64-row tile (and everything of the 256-row iteration behind it) is mostly padding.
# ---------------------------------------------------------------------------------------------
LAYOUT_RAYS = 5
LAYOUT_BG = 37
LAYOUT_SHAPE = dict(num_coarse_samples=8, num_fine_samples=6, num_nerf_point_freqs=4, use_stratified_sampling=True)
MLP_LAYOUTS = {
    'depth6': dict(nerf_trunk_depth=6),                                                                  # identities at layers 6, 7
    'depth4-noskip-warp': dict(nerf_trunk_depth=4, nerf_skips=(), use_warp=True, num_warp_freqs=4),      # zero posenc rows at layer 4
    'depth2-nocond': dict(nerf_trunk_depth=2, use_viewdirs=False),                                       # trunk and bottleneck identities
    'skip2-depth6-warp': dict(nerf_skips=(2,), nerf_trunk_depth=6, use_warp=True, num_warp_freqs=4),     # relaid, identities at 2, 3
    'skip1-depth5': dict(nerf_skips=(1,), nerf_trunk_depth=5),                                           # relaid, identities at 1, 2, 3
    'skip3-depth5-noviewdirs': dict(nerf_skips=(3,), nerf_trunk_depth=5, use_viewdirs=False),            # relaid, no bottleneck
    'w96-rgb40': dict(nerf_trunk_width=96, nerf_rgb_branch_width=40),
    'w128-rgb128': dict(nerf_trunk_width=128, nerf_rgb_branch_width=128),                                # equal widths
    'depth6-alphacond': dict(nerf_trunk_depth=6, use_appearance_metadata=True, use_alpha_condition=True),
}
_WARP = dict(use_warp=True, num_warp_freqs=4, num_warp_features=8)
WARP_LAYOUTS = {
    '5x96': dict(_WARP, warp_trunk_depth=5, warp_trunk_width=96),
    '3x64': dict(_WARP, warp_trunk_depth=3, warp_trunk_width=64),                                        # never reaches its skip
    '1x128': dict(_WARP, warp_trunk_depth=1, warp_trunk_width=128),
    '6x40': dict(_WARP, warp_trunk_depth=6, warp_trunk_width=40),
    'translation-4x80': dict(_WARP, warp_field_type='translation', warp_trunk_depth=4, warp_trunk_width=80),
    'translation-6x128': dict(_WARP, warp_field_type='translation'),
    'se3-6x128-time': dict(_WARP, warp_metadata_encoder_type='time'),
}
LAYOUT_TIME_ALPHA = 1.0
