"""ModelConfig.nerf_rgb_branch_depth = 2..4 (configs.py:55, modules.py:129-134) on the GPU, float32 mode: the extra 128 x 128 layers
of the rgb branch in the 64-row chain kernels (csrc/mlp_chain.hip), their weight gradients, the caller's tree, the refused modes and
the drivers.

  * forward + every gradient leaf against the float64 oracle pinned to the HIP path's ReLU branches (tests/helpers.py run_pinned);
    helpers.gpu_relu_masks decodes rgb layer 0 ("bits_rgbh"), the wrapper below appends layers 1.. from "bits_rgbx";
  * NerfModel.apply against arrays the unmodified reference produced with a deeper branch (tests/golden/ref_nerf_rgbdepth*.npz);
  * the result of a ray does not depend on the launch it rides in (a handle with a deeper branch keeps the 64-row kernels where a
    one-layer model takes the 32-row tiling);
  * bfloat16 / split-bf16 modes are refused by name; the graph-replayed train step equals the eager one; train.py / eval.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import helpers as H  # noqa: E402
from oracle import nerfies_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HERE = os.path.dirname(os.path.abspath(__file__))


def _np(t):
  return t.detach().cpu().double().numpy()


@pytest.fixture
def all_rgb_masks(monkeypatch):
  """helpers.gpu_relu_masks with the masks of EVERY rgb layer under '<level>/MLP_1' (the oracle's hook index = the layer)."""
  first_layer_only = H.gpu_relu_masks

  def masks(model, spec, num_rays, nbg=0, elastic=False):
    out = first_layer_only(model, spec, num_rays, nbg, elastic)
    nx = spec.nerf_rgb_branch_depth - 1
    if nx > 0:
      ws = model.workspace(num_rays, True, H.DEV, nbg, elastic)
      levels = [('coarse', 0, num_rays * spec.num_coarse_samples)]
      if spec.num_fine_samples > 0:
        levels.append(('fine', 1, num_rays * (spec.num_coarse_samples + spec.num_fine_samples)))
      for name, lv, rows in levels:
        nt = (rows + 63) // 64
        m = H._decode_bits(H._ws_words(model, ws, 'bits_rgbx', lv, nx * nt * 4 * 64), nx, nt, 1, rows)
        out[f'{name}/MLP_1'] = out[f'{name}/MLP_1'] + [m[i][:, :spec.nerf_rgb_branch_width] for i in range(nx)]
    return out
  monkeypatch.setattr(H, 'gpu_relu_masks', masks)


def _background(spec, nbg, seed=5):
  g = torch.Generator().manual_seed(seed)
  return {'points': torch.rand(nbg, 3, generator=g).double() - 0.5, 'warp_ids': torch.randint(0, spec.num_warp_embeddings, (nbg,), generator=g),
          'noise': 0.001 * torch.randn(nbg, 3, generator=g).double(), 'weight': 1.0}


# (ModelSpec keywords, rays, warp alpha, elastic + 37 background points)
PINNED = {
    'depth2_camera': (dict(nerf_rgb_branch_depth=2, num_nerf_point_freqs=6, num_coarse_samples=16, num_fine_samples=16,
                           use_camera_metadata=True), 40, 0.0, False),
    'depth3_w72x40': (dict(nerf_rgb_branch_depth=3, nerf_trunk_width=72, nerf_rgb_branch_width=40, num_nerf_point_freqs=4,
                           num_coarse_samples=16, num_fine_samples=8), 19, 0.0, False),
    'depth2_nocond': (dict(nerf_rgb_branch_depth=2, use_viewdirs=False, num_nerf_point_freqs=4, num_coarse_samples=16,
                           num_fine_samples=8), 17, 0.0, False),
    'depth2_se3_alphacond_elastic_bg': (dict(nerf_rgb_branch_depth=2, use_warp=True, num_warp_freqs=4, use_appearance_metadata=True,
                                             use_alpha_condition=True, num_nerf_point_freqs=6, num_coarse_samples=16,
                                             num_fine_samples=16), 21, 2.5, True),
    'depth4_translation': (dict(nerf_rgb_branch_depth=4, use_warp=True, warp_field_type='translation', num_warp_freqs=5,
                                num_nerf_point_freqs=8, num_coarse_samples=24, num_fine_samples=24), 23, 3.0, False),
    'depth2_skip5': (dict(nerf_rgb_branch_depth=2, nerf_skips=(5,), num_nerf_point_freqs=6, num_coarse_samples=16,
                          num_fine_samples=16), 20, 0.0, False),
}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_deeper_rgb_branch_forward_and_gradients(name, all_rgb_masks):
  """Loss 1e-5, rendered outputs 1e-4, every gradient leaf within helpers.grad_tol of its max-abs against the pinned float64 oracle,
  inside the project's tie caps (helpers.FLIP_FRACTION / FLIP_PRE)."""
  kw, B, alpha, regs = PINNED[name]
  spec = O.ModelSpec(use_stratified_sampling=True, **kw)
  extra = {}
  if regs:
    extra = dict(elastic={'weight': 0.01, 'reduce_method': 'weight'}, background=_background(spec, 37))
  r = H.run_pinned(spec, B, alpha, seed=43, **extra)
  H.assert_pinned(r, f'{name} B={B}')
  H.assert_forward(r, spec)
  D, w = spec.nerf_rgb_branch_depth, spec.nerf_rgb_branch_width
  names = [n for n, _, _ in r['model'].layout.entries]
  shapes = {n: tuple(sh) for n, _, sh in r['model'].layout.entries}
  for lv in ('coarse', 'fine'):
    base = f'nerf_mlps_{lv}/MLP_1'
    assert shapes[f'{base}/hidden_0/kernel'] == (spec.nerf_trunk_width + spec.rgb_cond_width, w)
    want = [f'{base}/hidden_{i}/{leaf}' for i in range(D) for leaf in ('kernel', 'bias')] + [f'{base}/logit/kernel', f'{base}/logit/bias']
    at = names.index(want[0])
    assert names[at:at + len(want)] == want                  # flax order: hidden_0, hidden_1, .., logit
    assert f'{base}/hidden_{D}/kernel' not in shapes
    for i in range(1, D):
      assert shapes[f'{base}/hidden_{i}/kernel'] == (w, w) and shapes[f'{base}/hidden_{i}/bias'] == (w,)
      for leaf in ('kernel', 'bias'):
        g = H.leaf(r['got'], f'{base}/hidden_{i}/{leaf}')
        assert g.abs().max().item() > 0, (lv, i, leaf)
        assert f'{base}/hidden_{i}/{leaf}' in r['errs']        # ... and it was compared with the oracle's


RGB_DEPTH_CASES = {   # tests/golden/make_reference_vectors_rgb_depth.py::RGB_DEPTH_CASES (3 rays, 8 + 6 samples, F_p = 4, stratified)
    'rgbdepth2': (dict(nerf_rgb_branch_depth=2, use_camera_metadata=True), 0.0),
    'rgbdepth3_w72x40': (dict(nerf_rgb_branch_depth=3, nerf_trunk_width=72, nerf_rgb_branch_width=40), 0.0),
    'rgbdepth2_nocond': (dict(nerf_rgb_branch_depth=2, use_viewdirs=False), 0.0),
    'rgbdepth2_warp_alphacond': (dict(nerf_rgb_branch_depth=2, use_warp=True, num_warp_freqs=4, use_appearance_metadata=True,
                                      use_alpha_condition=True), 2.5),
}


@pytest.mark.parametrize('name', sorted(RGB_DEPTH_CASES))
def test_apply_against_the_reference_run_with_a_deeper_rgb_branch(name):
  """One hop: NerfModel.apply on the rays, parameters and uniforms the unmodified reference was run on (no oracle in between; it
  only rebuilds the seeded parameter tree and batch).  Tolerances of tests/test_gpu_reference_onehop.py."""
  kw, alpha = RGB_DEPTH_CASES[name]
  r = dict(np.load(os.path.join(HERE, 'golden', f'ref_nerf_{name}.npz'), allow_pickle=False))
  spec = O.ModelSpec(num_coarse_samples=8, num_fine_samples=6, num_nerf_point_freqs=4, use_stratified_sampling=True, **kw)
  seed = int(r['seed'])
  params = O.init_params(spec, seed=seed, trained_like=True)
  batch = O.synthetic_batch(3, seed=seed + 1)
  model, fp = H.gpu_model(spec, params, 3)
  rngs = {'coarse': torch.tensor(r['t_rand']).float().to(DEV), 'fine': torch.tensor(r['u']).float().to(DEV)}
  out = model.apply({'params': fp}, H.gpu_batch(batch), {'alpha': alpha}, rngs=rngs, return_weights=True, return_points=spec.use_warp)
  worst = {}
  for lv in ('coarse', 'fine'):
    for k in ('rgb', 'depth', 'acc', 'weights'):
      got, want = _np(out[lv][k]), r[f'{lv}/{k}']
      worst[k] = max(worst.get(k, 0.0), float(np.abs(got - want).max()))
      np.testing.assert_allclose(got, want, atol=1e-4, err_msg=f'{name} {lv}/{k}')
    if spec.use_warp:
      np.testing.assert_allclose(_np(out[lv]['warped_points']), r[f'{lv}/warped_points'], atol=1e-4, err_msg=f'{name} {lv}/warped_points')
  print(f'one-hop {name}: max |hip - reference| ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))


def test_the_result_does_not_depend_on_the_launch_size():
  """The depth-2 camera-code model at 64 + 128 samples (192 samples per fine ray: not a divisor of the 64-row tile), inference: at 128
  rays -- where a one-layer model's forward takes the 32-row tiling (128 and 384 tiles for 512 workgroup slots; a deeper branch keeps
  the 64-row kernels) -- and at 1024 + 37 rays with a ragged last tile.  A 64-ray subset of each within 1e-4 of the float64 oracle,
  and the 128 rays rendered alone equal to the same rays at the head of the large batch."""
  spec = O.ModelSpec(nerf_rgb_branch_depth=2, use_camera_metadata=True)
  assert (spec.num_coarse_samples, spec.num_fine_samples) == (64, 128)
  params = O.init_params(spec, seed=47, trained_like=True)
  big = O.synthetic_batch(1024 + 37, seed=48)
  take = lambda b, sl: {k: (v[sl] if torch.is_tensor(v) else {kk: vv[sl] for kk, vv in v.items()}) for k, v in b.items()}
  model, fp = H.gpu_model(spec, params, 128)
  outs = {}
  for n, subset in ((128, slice(32, 96)), (1024 + 37, slice(1024 + 37 - 64, 1024 + 37))):
    b = take(big, slice(0, n))
    out = model.apply({'params': fp}, H.gpu_batch(b), {'alpha': 0.0})
    outs[n] = out
    with torch.no_grad():
      ret = O.nerf_model_apply(params, spec, take(b, subset), 0.0)
    for lv in ('coarse', 'fine'):
      for k in ('rgb', 'depth', 'acc'):
        got, want = _np(out[lv][k])[subset], ret[lv][k].numpy()
        np.testing.assert_allclose(got, want, atol=1e-4, err_msg=f'{n} rays {lv}/{k}')
    print(f'{n} rays: max |hip - oracle| fine rgb {np.abs(_np(out["fine"]["rgb"])[subset] - ret["fine"]["rgb"].numpy()).max():.2e}')
  for lv in ('coarse', 'fine'):
    for k in ('rgb', 'depth', 'acc'):
      assert torch.equal(outs[128][lv][k], outs[1024 + 37][lv][k][:128]), (lv, k)
  from nerfies_amd import lib as L
  with pytest.raises(L.NrfError, match='64-row'):
    model.set_chain_tile_rows(32)


def test_bf16_modes_are_refused_by_name():
  from nerfies_amd import lib as L
  spec = O.ModelSpec(nerf_rgb_branch_depth=2, num_coarse_samples=16, num_fine_samples=16, num_nerf_point_freqs=4)
  B = 16
  model, fp = H.gpu_model(spec, O.init_params(spec, seed=3, trained_like=True), B)
  gb = H.gpu_batch(O.synthetic_batch(B, seed=4))
  for mode in ('mlp', True):
    with pytest.raises(L.NrfError, match='rgb'):
      model.loss_and_grad(fp, gb, warp_extra={'alpha': 0.0}, bf16=mode)
  with pytest.raises(L.NrfError, match='rgb'):
    model.apply({'params': fp}, gb, {'alpha': 0.0}, bf16='x3')
  with pytest.raises(L.NrfError, match='rgb'):
    model.apply({'params': fp}, gb, {'alpha': 0.0}, bf16=True)
  grad, stats = model.loss_and_grad(fp, gb, warp_extra={'alpha': 0.0})   # the float32 mode runs
  assert torch.isfinite(grad).all() and torch.isfinite(stats[:5]).all()


def test_graph_replay_equals_eager_at_depth_2():
  """training.GraphedTrainStep of a depth-2 model against the eager training.train_step from the same state, two steps at B = 128:
  the gates of tests/test_gpu_graph_step.py::test_graph_replay_equals_eager_config_a_shape."""
  from nerfies_amd import models, training

  class Cfg:
    num_coarse_samples, num_fine_samples, num_nerf_point_freqs = 64, 128, 8
    sigma_activation, use_stratified_sampling, use_viewdirs = 'softplus', True, True
    nerf_rgb_branch_depth = 2
  B = 128
  pair = []
  for _ in range(2):   # same seed -> identical initial parameters
    model, fp = models.construct_nerf(11, Cfg, B, [0, 1, 2, 3], [0, 1], [0, 1, 2, 3], 0.05, 1.0, device='cuda:0')
    pair.append((model, training.TrainState(optimizer=training.Optimizer(fp), warp_alpha=1.5)))
  (me, se), (mg, sg) = pair
  assert torch.equal(sg.optimizer.target.flat, se.optimizer.target.flat)
  assert mg.layout.shape_of('nerf_mlps_fine/MLP_1/hidden_1/kernel') == (128, 128)

  def batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {'origins': (torch.rand(B, 3, generator=g) - 0.5).to('cuda:0'),
            'directions': torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1).to('cuda:0'),
            'rgb': torch.rand(B, 3, generator=g).to('cuda:0'), 'metadata': {}}
  batches = [batch(70 + k) for k in range(2)]
  gstep = training.GraphedTrainStep(mg, sg, batches[0], training.ScalarParams(learning_rate=1e-3))
  key = 7
  for k in range(2):
    sp = training.ScalarParams(learning_rate=1e-3 * 0.5 ** k)
    se, st_e, next_key = training.train_step(me, key, se, batches[k], sp)
    st_g = gstep(key, scalar_params=sp, batch=batches[k])
    key = next_key
    assert abs(st_e['fine']['loss/rgb'].item() - st_g['fine']['loss/rgb'].item()) < 1e-7
    ge, gg = se.optimizer.grad.cpu(), sg.optimizer.grad.cpu()
    worst = 0.0
    for name, off, shape in mg.layout.entries:
      n = int(np.prod(shape))
      x, y = gg[off:off + n], ge[off:off + n]
      scale = y.abs().max().item()
      if scale > 0:
        worst = max(worst, (x - y).abs().max().item() / scale)
        assert (x - y).abs().max().item() <= 2e-5 * scale, (k, name, (x - y).abs().max().item(), scale)
    assert ge[mg.layout.by_name['nerf_mlps_fine/MLP_1/hidden_1/kernel'][0]:][:128 * 128].abs().max().item() > 0
    for dst, src in ((sg.optimizer.target.flat, se.optimizer.target.flat), (sg.optimizer.m, se.optimizer.m), (sg.optimizer.v, se.optimizer.v)):
      dst.copy_(src)   # every step's comparison is of ONE step from the same state
    print(f'[graphed step, depth 2] step {k}: worst gradient leaf {worst:.1e} of its max-abs vs eager')
  assert sg.optimizer.step == se.optimizer.step == 2


GIN = """
max_steps = 40
batch_size = 256
eval_batch_size = 128
init_lr = 0.002
final_lr = 0.001
elastic_init_weight = 0.001
LR = {'type': 'exponential', 'initial_value': %init_lr, 'final_value': %final_lr, 'num_steps': %max_steps}
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
ModelConfig.nerf_rgb_branch_depth = 2
TrainConfig.batch_size = %batch_size
TrainConfig.max_steps = %max_steps
TrainConfig.lr_schedule = %LR
TrainConfig.warp_alpha_schedule = ('linear', 0.0, 4.0, 20)
TrainConfig.use_elastic_loss = True
TrainConfig.elastic_loss_weight_schedule = ('constant', %elastic_init_weight)
TrainConfig.use_background_loss = True
TrainConfig.background_loss_weight = 1.0
TrainConfig.background_points_batch_size = 32
TrainConfig.print_every = 10
TrainConfig.log_every = 10
TrainConfig.save_every = 20
EvalConfig.chunk = %eval_batch_size
EvalConfig.eval_once = True
EvalConfig.num_train_eval = 1
EvalConfig.num_val_eval = 1
"""   # tests/test_gpu_datasets.py::test_train_and_eval_drivers_end_to_end's, plus the rgb branch depth


def test_drivers_train_resume_and_eval_at_depth_2(tmp_path, capsys):
  import eval as eval_driver
  import train as train_driver
  from nerfies_amd import checkpoints, datasets, gin_lite as gin
  cap, exp = str(tmp_path / 'cap'), str(tmp_path / 'exp')
  datasets.write_synthetic_scene(cap, num_frames=4, size=(24, 16))
  cfg = tmp_path / 'run.gin'
  cfg.write_text(GIN)
  args = ['--base_folder', exp, '--data_dir', cap, '--gin_configs', str(cfg)]
  gin.clear_config()
  state = train_driver.main(args + ['--max_steps', '20'])
  assert state.optimizer.step == 20 and os.path.exists(os.path.join(exp, 'checkpoints', 'checkpoint_20'))
  assert 'ModelConfig.nerf_rgb_branch_depth = 2' in open(os.path.join(exp, 'config.gin')).read()
  gin.clear_config()
  state = train_driver.main(args)                                    # restores checkpoint_20, runs to 40
  assert state.optimizer.step == 40
  assert 'Starting training at step 21' in capsys.readouterr().out
  params = state.optimizer.target.tree
  assert tuple(params['nerf_mlps_fine']['MLP_1']['hidden_1']['kernel'].shape) == (128, 128)
  assert tuple(params['nerf_mlps_coarse']['MLP_1']['hidden_1']['bias'].shape) == (128,)
  restored = checkpoints.restore_checkpoint(os.path.join(exp, 'checkpoints'), state)
  assert restored.optimizer.step == 40
  assert torch.equal(restored.optimizer.target.tree['nerf_mlps_fine']['MLP_1']['hidden_1']['kernel'].cpu(),
                     params['nerf_mlps_fine']['MLP_1']['hidden_1']['kernel'].cpu())
  scal = [json.loads(l) for l in open(os.path.join(exp, 'summaries', 'train', 'scalars.jsonl'))]
  loss = {r['step']: r['value'] for r in scal if r.get('tag') == 'loss/rgb/fine'}
  assert sorted(loss) == [10, 20, 30, 40] and loss[40] < loss[10], loss
  gin.clear_config()
  res = eval_driver.main(args)
  assert set(res) == {'val', 'train'} and np.isfinite(res['val']['psnr']) and np.isfinite(res['train']['mse'])
  gin.clear_config()
  with pytest.raises(SystemExit, match='rgb branch'):                # the split-bf16 chains run a one-layer branch
    eval_driver.main(args + ['--bf16', 'x3'])
  gin.clear_config()
  with pytest.raises(SystemExit, match='rgb branch'):
    train_driver.main(args + ['--bf16'])
  gin.clear_config()
