"""SE3 trunk on bfloat16 operands (csrc/warp_bf16.hip; NRF_FLAG_BF16 with the warp field, BASELINE configs[3]).

The reference has no reduced-precision mode (warping.py:264-288 runs in float32), so parity is established as for the NeRF MLPs
(tests/test_gpu_bf16_train.py):
  1. GIVEN THE KERNELS' OWN STASH, in float64 with the same roundings: every stashed quantity of every pass through the field
     (coarse / fine samples, background points, the three tangents per coarse sample) is recomputed from the stashed quantity in
     front of it -- trunk input from the points, h_{l+1} from h_l, the head outputs (w, v) from h_6, dpre_{l-1} from dpre_l and
     the ReLU mask, the warp leaves' gradients from the (X, dY) stashes summed over the passes.  This pins layouts, masks, weight
     streams, the panel pipeline and the wgrad plumbing without the tie amplification an end-to-end comparison suffers.
  2. AGAINST THE float32 TRUNK on identical rays (bf16='mlp' keeps it in float32, everything else equal): warped points, loss,
     elastic / background loss values (within 2 %), every gradient leaf's direction (cos >= 0.97).
The end-to-end training gate (held-out PSNR with the warp on) is tests/test_gpu_bf16_convergence.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from oracle import nerfies_oracle as O  # noqa: E402
import helpers as H  # noqa: E402
from bf16_reference import ALPHA, warp_setup as _setup, check_warp_given_the_stash  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_bf16_warp_stash_chain_and_leaf_gradients_given_the_stash():
  B, nbg = 21, 100
  check_warp_given_the_stash(_setup(B, nbg=nbg, use_camera_metadata=True), nbg)


@pytest.mark.parametrize('kw,head_scale', [(dict(num_warp_freqs=6, use_camera_metadata=True), 0.02),
                                           (dict(num_nerf_point_freqs=10, num_coarse_samples=64, num_fine_samples=64), 0.02),
                                           (dict(num_warp_freqs=6, use_camera_metadata=True), 1.0),
                                           # TranslationField (warping.py:62-199) = the trunk with a zero rotation head
                                           (dict(warp_field_type='translation', num_warp_freqs=5), 0.05),
                                           # codes from modules.TimeEncoder (one row per ray) instead of the GLO table
                                           (dict(warp_metadata_encoder_type='time', num_warp_freqs=6), 0.02)])
def test_bf16_warp_against_the_float32_trunk(kw, head_scale):
  """What the bfloat16 trunk costs next to the float32 trunk, everything else (bf16 NeRF MLPs, rays, uniforms) equal.

  The trunk's bf16 operands move a warped point by ~5e-4 of its displacement (rms; measured below).  Two regimes:
  * head_scale 0.02 -- displacements of ~0.1 scene units, what a capture's deformation field looks like: the perturbation is
    ~5e-5, the NeRF posenc (2^(F_p - 1)) turns it into ~1e-2 rad at the top band, and every gradient leaf keeps its direction;
  * head_scale 1 -- the oracle's "trained-like" heads, which throw points ~4 scene sizes away (built to expose indexing bugs, not
    to resemble a scene): the same relative error is 2e-3 absolute = ~1 rad at the top band, the rendered colours and with
    them the upstream gradient d loss / d x' change by O(1), and the gradient directions of the warp field decorrelate.  That is
    the 2^(F_p - 1) amplification any perturbation of x' meets (two float32 evaluation orders differ by the same factor times 1e-7,
    tests/test_gpu_pinned.py), not an error of the kernels -- those are pinned by the given-the-stash test above; here only the
    values that do not pass through the NeRF posenc are compared (warped points, regulariser values)."""
  from nerfies_amd import params as P
  time_enc = kw.get('warp_metadata_encoder_type') == 'time'
  B, nbg = 96, (0 if time_enc else 512)   # the background points carry warp ids, which a time-encoded field does not have
  wextra = {'alpha': ALPHA, 'time_alpha': 1.0} if time_enc else {'alpha': ALPHA}
  spec, p, b, model, fp, rngs, bg = _setup(B, seed=11, nbg=nbg, head_scale=head_scale, **kw)
  gb = H.gpu_batch(b)
  realistic = head_scale < 1.0
  # inference: warped points
  o16 = model.apply({'params': fp}, gb, wextra, rngs=rngs, return_points=True, bf16=True)
  o32 = model.apply({'params': fp}, gb, wextra, rngs=rngs, return_points=True, bf16='mlp')
  for lv in ('coarse', 'fine'):
    disp = (o32[lv]['warped_points'] - o32[lv]['points']).abs().max().item()
    dxs = (o16[lv]['warped_points'] - o32[lv]['warped_points']).abs()
    dx, rms = dxs.max().item(), dxs.pow(2).mean().sqrt().item()
    print(f"[bf16 vs f32 SE3 trunk, heads x {head_scale}, {lv}] max |x' - x| {disp:.4f}; |x'_bf16 - x'_f32| max {dx:.2e} rms {rms:.2e}; "
          f"max |rgb_bf16 - rgb_f32| {(o16[lv]['rgb'] - o32[lv]['rgb']).abs().max().item():.2e}")
    assert disp > 1e-3 and dx < 2e-2 * disp + 1e-5 and rms < 2e-3 * disp + 1e-6, (lv, dx, rms, disp)
    if realistic:
      assert (o16[lv]['rgb'] - o32[lv]['rgb']).abs().max().item() < 2e-2
  # training: loss, regulariser values, gradient directions
  extra = dict(warp_extra=wextra, rngs=rngs, background=bg, elastic={'weight': 0.01, 'reduce_method': 'weight'})
  g32, s32 = model.loss_and_grad(fp, gb, bf16='mlp', **extra)
  g32, s32 = g32.clone(), s32.clone()
  g16, s16 = model.loss_and_grad(fp, gb, bf16=True, **extra)
  assert torch.isfinite(g16).all() and torch.isfinite(s16).all()
  assert abs(s16[4].item() - s32[4].item()) < 1e-3 + 2e-2 * abs(s32[4].item())
  for k, what in ((5, 'background loss'), (6, 'elastic loss'), (7, 'elastic residual'))[(1 if time_enc else 0):]:
    assert abs(s16[k].item() - s32[k].item()) < 2e-2 * abs(s32[k].item()) + 1e-9, (what, s16[k].item(), s32[k].item())
  t32, t16 = P.tree_from_flat(g32.cpu(), model.layout), P.tree_from_flat(g16.cpu(), model.layout)
  cos_min, cos_warp, table = 1.0, 1.0, []
  for path, a in O.tree_leaves_with_path(t32):
    c = torch.nn.functional.cosine_similarity(a.flatten().double(), H.leaf(t16, path).flatten().double(), dim=0).item()
    table.append((path, c))
    cos_min = min(cos_min, c)
    if path.startswith('warp_field'):
      cos_warp = min(cos_warp, c)
  print(f'[bf16 vs f32 SE3 trunk {kw}, heads x {head_scale}] loss {s16[4].item():.6f} / {s32[4].item():.6f}, elastic {s16[6].item():.4e} / '
        f'{s32[6].item():.4e}, background {s16[5].item():.4e} / {s32[5].item():.4e}; min leaf cosine {cos_min:.4f} (warp field {cos_warp:.4f})')
  if realistic:
    assert cos_warp > 0.97 and cos_min > 0.97, '\n'.join(f'    {c:.4f}  {path}' for path, c in table)


def test_bf16_warp_inference_renderer_and_opt_out():
  """GraphedChunkRenderer in the bf16 mode renders through the bf16 trunk; the Jacobian output keeps the float32 trunk."""
  from nerfies_amd import evaluation
  spec, p, b, model, fp, rngs, _ = _setup(64, seed=3, use_stratified_sampling=False)
  gb = {k: v for k, v in H.gpu_batch(b).items() if k != 'rgb'}
  fn = evaluation.GraphedChunkRenderer(model, bf16=True)
  a = fn(0, 1, fp, gb, {'alpha': ALPHA})
  direct = model.apply({'params': fp}, gb, {'alpha': ALPHA}, bf16=True)
  np.testing.assert_array_equal(a['fine']['rgb'].cpu().numpy(), direct['fine']['rgb'].cpu().numpy())
  j16 = model.apply({'params': fp}, gb, {'alpha': ALPHA}, return_warp_jacobian=True, bf16=True)
  j32 = model.apply({'params': fp}, gb, {'alpha': ALPHA}, return_warp_jacobian=True)
  np.testing.assert_allclose(j16['coarse']['warp_jacobian'].cpu().numpy(), j32['coarse']['warp_jacobian'].cpu().numpy(), atol=1e-6)
