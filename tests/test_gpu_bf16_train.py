"""bf16 training path (NRF_FLAG_TRAIN | NRF_FLAG_BF16; BASELINE configs[3] "bf16 MLP with fp32 composite"): forward with
the bf16 stash, bf16 dgrad chain, bf16 wgrad with LDS transpose reads (csrc/mlp_bf16.hip, csrc/wgrad_bf16.hip).

The reference has no reduced-precision mode, so parity is established in two steps:
  1. against the float64 oracle evaluated with the SAME roundings -- activations and weights rounded to bfloat16 as GEMM
     operands, the back-propagated pre-activation gradients rounded to bfloat16 before they are used (for dX, dW and db
     alike), biases / the per-ray condition term / everything outside the MLP exact -- the HIP path must agree per leaf to
     1e-2 of the leaf's max-abs entry (measured ~1e-3: fp32 vs fp64 accumulation and one-ulp bf16 ties).  This pins the
     kernels' dataflow (stash layout, masks, transposes) independently of how much bf16 itself costs;
  2. against the fp32 path on identical rays: what bf16 costs -- loss within 1e-3, every gradient leaf's direction within
     cos >= 0.99 -- and a short training run: PSNR on held-out rays within 0.1 dB of the fp32 run (SURVEY 8d gate)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from oracle import nerfies_oracle as O  # noqa: E402
import helpers as H  # noqa: E402
from bf16_reference import MLP, WARP_ALPHA, mlp_setup as _setup, check_forward_and_stash, check_backward_given_the_stash  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the step-1 checks below (tests/bf16_reference.py, shared with the other layouts of tests/test_gpu_bf16_layouts.py) pin the NeRF-MLP
# chain against an oracle that rounds exactly what that chain rounds: they run the mode that keeps the SE3 trunk in float32
# (MLP: bf16='mlp' = NRF_FLAG_BF16 | NRF_FLAG_WARP_F32); the bfloat16 trunk has its own checks in tests/test_gpu_bf16_warp.py, and the
# end-to-end gates (gradient direction, PSNR) run the full bf16 mode


CASES = [(37, {}), (401, {}), (50, dict(num_nerf_point_freqs=10, use_camera_metadata=True)),
         (24, dict(nerf_trunk_width=128, nerf_rgb_branch_width=64, num_coarse_samples=32, num_fine_samples=32)),
         (45, dict(use_warp=True, num_warp_freqs=6, use_camera_metadata=True, num_coarse_samples=48, num_fine_samples=48)),
         (21, dict(use_warp=True, num_nerf_point_freqs=10, num_coarse_samples=32, num_fine_samples=32)),
         (3, dict(num_coarse_samples=8, num_fine_samples=5)),       # 24 / 39 rows: one workgroup iteration, most waves padding
         (1, dict(num_coarse_samples=16, num_fine_samples=0))]      # a single ray, coarse level only


@pytest.mark.parametrize('B,kw', CASES)
def test_bf16_forward_and_stash_match_the_rounded_oracle(B, kw):
  check_forward_and_stash(_setup(B, **kw))


@pytest.mark.parametrize('B,kw', CASES)
def test_bf16_backward_matches_float64_given_the_stash(B, kw):
  check_backward_given_the_stash(_setup(B, **kw))


# warp on: bf16='mlp' (NeRF MLPs in bf16, SE3 trunk float32) -- this test prices the MLP chain; the bf16 trunk in front of the
# 2^(F_p - 1) posenc is priced separately (tests/test_gpu_bf16_warp.py: realistic and "trained-like" head scales)
@pytest.mark.parametrize('kw,cos_floor', [({}, 0.99), (dict(use_warp=True, num_warp_freqs=6), 0.97)])
def test_bf16_gradient_against_the_fp32_path(kw, cos_floor):
  from nerfies_amd import params as P
  B = 128
  spec, p, b, t_rand, u, model, fp, rngs = _setup(B, seed=9, **kw)
  gb = H.gpu_batch(b)
  extra = dict(warp_extra={'alpha': WARP_ALPHA}, rngs=rngs)
  if kw:   # the regularisers' algebra (exp_se3, SVD) stays float32; the trunk they differentiate runs in the call's mode
    extra['elastic'] = {'weight': 0.01, 'reduce_method': 'weight'}
  g32, s32 = model.loss_and_grad(fp, gb, **extra)
  g32, s32 = g32.clone(), s32.clone()
  g16, s16 = model.loss_and_grad(fp, gb, bf16=MLP if kw else True, **extra)
  assert torch.isfinite(g16).all()
  assert abs(s16[4].item() - s32[4].item()) < 1e-3
  t32, t16 = P.tree_from_flat(g32.cpu(), model.layout), P.tree_from_flat(g16.cpu(), model.layout)
  cos_min = 1.0
  for path, a in O.tree_leaves_with_path(t32):
    c = torch.nn.functional.cosine_similarity(a.flatten().double(), H.leaf(t16, path).flatten().double(), dim=0).item()
    cos_min = min(cos_min, c)
    assert c > cos_floor, (path, c)
  print(f'[bf16 vs fp32 gradients {kw}] loss {s16[4].item():.6f} / {s32[4].item():.6f}, min leaf cosine {cos_min:.5f}')
  # the two training modes share the flat layout / Adam: switching per step is allowed and the fp32 result is unchanged
  g32b, _ = model.loss_and_grad(fp, gb, **extra)
  assert (g32b - g32).abs().max().item() <= 1e-6 * g32.abs().max().item()   # (atomics in the per-ray sums: not bitwise)


def _scene_rgb(o, d):
  """a smooth view-dependent target the network can fit"""
  return torch.sigmoid(torch.stack([2.0 * torch.sin(3.0 * o[:, 0] + 2.0 * d[:, 1]), 2.0 * torch.cos(2.0 * o[:, 1] - 3.0 * d[:, 2]),
                                    1.5 * torch.sin(4.0 * o[:, 2] + d[:, 0])], -1))


def test_bf16_training_reaches_the_fp32_psnr():
  """SURVEY 8d gate for the bf16 mode.  400 Adam steps on the same ray stream from the same init, PSNR of the trained
  models on held-out rays rendered by the fp32 eval path.  Two training runs that differ only in rounding diverge
  chaotically (two FLOAT32 runs with different stratified-sampling keys end +-0.3 dB apart on this scene), so the gate is
  one-sided and uses the fp32 spread as its reference: the bf16 run must reach the worse of two fp32 runs minus 0.1 dB,
  and its loss over the last 100 steps must be within 5 % of theirs."""
  from nerfies_amd import models, training
  B, K = 512, 400

  class Cfg:
    num_coarse_samples, num_fine_samples, num_nerf_point_freqs = 32, 64, 6
    sigma_activation, use_stratified_sampling, use_viewdirs = 'softplus', True, True
  g = torch.Generator().manual_seed(0)
  n_train = 64 * B
  o = (torch.rand(n_train + 4096, 3, generator=g) - 0.5).to(DEV)
  d = torch.nn.functional.normalize(torch.randn(n_train + 4096, 3, generator=g), dim=-1).to(DEV)
  rgb = _scene_rgb(o, d)
  em, _ = models.construct_nerf(7, type('E', (Cfg,), {'use_stratified_sampling': False}), 4096, [0], [0], [0], 0.05, 1.0, device=DEV)
  test = {'origins': o[n_train:], 'directions': d[n_train:], 'metadata': {}}
  runs = {}
  for mode, key0 in (('f32', 1), ('f32b', 1001), ('bf16', 1)):
    model, fp = models.construct_nerf(7, Cfg, B, [0], [0], [0], 0.05, 1.0, device=DEV)
    state = training.TrainState(optimizer=training.Optimizer(fp))
    sp = training.ScalarParams(learning_rate=1e-3)
    key, losses = key0, []
    for k in range(K):
      i0 = (k % 64) * B
      batch = {'origins': o[i0:i0 + B], 'directions': d[i0:i0 + B], 'rgb': rgb[i0:i0 + B], 'metadata': {}}
      state, stats, key = training.train_step(model, key, state, batch, sp, bf16=(mode == 'bf16'))
      losses.append(stats['fine']['loss/rgb'])
    losses = torch.stack(losses).cpu().numpy()
    psnr = {}
    for tag, kw in (('f32', {}), ('bf16', dict(bf16=True))):   # the same weights rendered by both inference modes
      out = em.apply({'params': fp}, test, {}, **kw)
      psnr[tag] = -10.0 * np.log10(((out['fine']['rgb'] - rgb[n_train:]) ** 2).mean().item())
    runs[mode] = (psnr, losses)
  (pa, la), (pb, lb), (p16, l16) = runs['f32'], runs['f32b'], runs['bf16']
  print(f'[bf16 training] held-out PSNR: fp32 runs {pa["f32"]:.3f} / {pb["f32"]:.3f} dB, bf16-trained {p16["f32"]:.3f} dB; the same weights '
        f'rendered with bf16 operands: {pa["bf16"] - pa["f32"]:+.3f} / {p16["bf16"] - p16["f32"]:+.3f} dB; mean loss of the last 100 steps '
        f'{la[-100:].mean():.5f} / {lb[-100:].mean():.5f} / {l16[-100:].mean():.5f}')
  assert min(pa['f32'], pb['f32']) > 20.0                       # the scene is learnt at all
  assert p16['f32'] >= min(pa['f32'], pb['f32']) - 0.1
  assert l16[-100:].mean() <= 1.05 * max(la[-100:].mean(), lb[-100:].mean())
  for psnr, _ in runs.values():                                  # inference-mode gate: bf16 rendering of given weights costs < 0.1 dB
    assert abs(psnr['bf16'] - psnr['f32']) <= 0.1


@pytest.mark.parametrize('kw', [dict(), dict(use_warp=True, num_warp_freqs=4, use_camera_metadata=True)])
def test_merged_wgrad_groups_give_the_same_gradient(kw):
  """NRF_OPT_BF16_WGRAD_MERGE (round 5): the skip layer as ONE weight-gradient group (X = [h4 | posenc], ten row blocks) and the
  bottleneck + alpha head as one (dY = [d bottleneck | d raw], nine column blocks) read the same bf16 stash as the default one
  group per matrix: every leaf -- in particular trunk/hidden_4's posenc rows and the alpha head's kernel, which come out of other
  slab windows -- must agree to float32 summation order (other segment boundaries), and the workspace is re-planned."""
  from nerfies_amd import lib as L
  spec = O.ModelSpec(num_coarse_samples=24, num_fine_samples=40, num_nerf_point_freqs=8, use_stratified_sampling=False, **kw)
  oparams = O.init_params(spec, seed=5, trained_like=True, dtype=torch.float32)
  B = 43
  batch = H.gpu_batch(O.synthetic_batch(B, seed=6, dtype=torch.float32))
  grads = []
  for merge in (0, 1):
    model, fp = H.gpu_model(spec, oparams, B)
    model.set_bf16_wgrad_merge(merge)   # also drops the cached workspaces (the option changes their size)
    g, st = model.loss_and_grad(fp, batch, warp_extra={'alpha': 2.0}, bf16=True)
    grads.append((g.clone(), st.clone(), model))
  (g0, s0, model), (g1, s1, _) = grads
  assert torch.equal(s0, s1)       # the forward / reverse chains do not depend on the option
  for name, off, shape in model.layout.entries:
    n = int(np.prod(shape))
    x, y = g0[off:off + n], g1[off:off + n]
    assert (x - y).abs().max().item() <= 2e-5 * x.abs().max().item() + 1e-12, (name, (x - y).abs().max().item(), x.abs().max().item())
  # switching the option on a LIVE model (one that has stepped: cached workspace of the other size) re-plans instead of reusing it
  model.set_bf16_wgrad_merge(1)
  g2, _ = model.loss_and_grad(fp, batch, warp_extra={'alpha': 2.0}, bf16=True)
  # same plan as the second model's: equal up to the float32 summation order of the atomically accumulated leaves (warp field, codes)
  assert (g2 - g1).abs().max().item() <= 2e-5 * g1.abs().max().item() + 1e-12
  with pytest.raises(L.NrfError):
    L.check(model.lib.nrf_set_option(model.handle, L.NRF_OPT_BF16_WGRAD_MERGE, 2), model.lib)
