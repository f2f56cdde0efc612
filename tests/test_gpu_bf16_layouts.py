"""The bfloat16 training chains on every trunk layout nrf_create accepts for them, leaf by leaf.

tests/test_gpu_bf16_train.py and tests/test_gpu_bf16_warp.py pin the default layout (8 x 256 NeRF trunk with its skip at 4 and a
bottleneck; 6 x 128 SE3 trunk with a GLO table) against a float64 recomputation with the same roundings.  nrf_create also lays
shallower, relaid, narrower and condition-free NeRF MLPs, warp trunks of 1..6 layers by 1..128 units, the TranslationField and the
time-encoded warp code on the same kernels (identity layers, zero posenc rows, zero padding, an internal bottleneck, a dead rotation
head); tests/test_gpu_contract.py runs the bf16 mode on those and asserts the cosine of the whole flattened gradient, which a few large
trunk kernels dominate.  Here the same-rounding references of tests/bf16_reference.py (proven against the float64 oracle on the CPU:
tests/test_bf16_reference_host.py) are held against the kernels on those layouts, with the bounds of the default layout:

  activations   max <= 2 % of the layer's scale, relative L2 <= 5e-3, >= 95 % of the elements within one bfloat16 ulp
  leaves        <= 5e-3 of the leaf's max-abs
  exact         identity layers equal to the stash in front of them, padded units zero (activations and dpre), the rotation head of a
                TranslationField zero, every leaf of the caller's tree covered by the reference (nothing of an identity in it)

at the smallest shapes that still cross a tile edge: 5 rays of 8 coarse + 6 fine samples (40 and 70 rows), 37 background points.
The figures of one run are in profiles/bf16_layout_parity.md."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bf16_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
_SETUPS = {}


def _mlp_setup(label):
  if label not in _SETUPS:   # one model per layout, shared by its three tests (nothing below writes to it)
    _SETUPS[label] = R.mlp_setup(R.LAYOUT_RAYS, **dict(R.LAYOUT_SHAPE, **R.MLP_LAYOUTS[label]))
  return _SETUPS[label]


@pytest.mark.parametrize('label', list(R.MLP_LAYOUTS))
def test_bf16_mlp_layout_forward_and_stash(label):
  setup = _mlp_setup(label)
  worst = R.check_forward_and_stash(setup)
  print(f'[bf16 MLP layout {label}] forward: worst activation {worst:.2e} of its layer\'s scale')


@pytest.mark.parametrize('label', list(R.MLP_LAYOUTS))
def test_bf16_mlp_layout_backward_given_the_stash(label):
  setup = _mlp_setup(label)
  spec, model = setup[0], setup[5]
  report = {}
  R.check_backward_given_the_stash(setup, report)
  print(f'[bf16 MLP layout {label}] backward: worst leaf {report["worst_leaf"][0]} {report["worst_leaf"][1]:.2e}')
  # the caller's tree is the reference's: its own trunk layers, a bottleneck only with a condition
  names = [n for n, _, _ in model.layout.entries]
  assert sum('nerf_mlps_coarse/MLP_0/' in n and n.endswith('kernel') for n in names) == spec.nerf_trunk_depth
  assert any('bottleneck' in n for n in names) == R.MlpLayout(spec).bottleneck


@pytest.mark.parametrize('label', list(R.MLP_LAYOUTS))
def test_bf16_mlp_layout_inference_renders_the_training_forward(label):
  R.check_inference_matches_training(_mlp_setup(label))


@pytest.mark.parametrize('label', list(R.WARP_LAYOUTS))
def test_bf16_warp_layout_given_the_stash(label):
  kw = dict(R.LAYOUT_SHAPE, **R.WARP_LAYOUTS[label])
  time = kw.get('warp_metadata_encoder_type') == 'time'
  nbg = 0 if time else R.LAYOUT_BG                      # the background points carry warp ids, which a time-encoded field does not have
  setup = R.warp_setup(R.LAYOUT_RAYS, nbg=nbg, **kw)
  elastic = kw.get('warp_field_type', 'se3') == 'se3'   # the elastic loss is the SE3 field's
  worst_act, worst = R.check_warp_given_the_stash(setup, nbg, elastic=elastic, time_alpha=R.LAYOUT_TIME_ALPHA if time else None)
  print(f'[bf16 warp layout {label}] worst activation {worst_act:.2e} of its layer\'s scale, worst leaf {worst[0]} {worst[1]:.2e}')
