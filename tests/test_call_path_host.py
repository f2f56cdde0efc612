"""The Python host's call path without a GPU: NerfModel.flags -> NerfModel._record -> models.CallRecord.  One function makes the
NRF_FLAG_* word, the workspace cache is keyed by the word the workspace is sized for, and `stash` / `generation` are declared
attributes.  The sizes are pinned to the commit before that refactor, which pins the flag word and the key's normalisation together:
a wrong bit or a wrong sharing rule asks the library for another size."""
import types

import pytest
import torch

B = 37   # no multiple of the 32- or 64-row tiles
WARP = dict(use_warp=True, warp_field_type='se3', num_warp_freqs=4)


def _model(**kw):
  """tests/test_ray_grads_host.py::_model."""
  from nerfies_amd import models
  cfg = types.SimpleNamespace(num_coarse_samples=8, num_fine_samples=6, num_nerf_point_freqs=4, use_stratified_sampling=False, **kw)
  model, _ = models.construct_nerf(0, cfg, 4, [0], [0], [0, 1], 0.1, 1.0, device='cpu')
  return model


# NerfModel.workspace(37, ...).numel() (float32 words) of the parent commit, for _model() / _model(**WARP).  They depend on the
# compute-unit count the handle plans for: 256, what a handle assumes until it has seen a device and what the MI355X reports.  To
# regenerate: check the parent commit out next to this one, build it, and print model.workspace(37, train, 'cpu', ...).numel() for the
# calls of _CALLS below.
_CALLS = {   # name -> (train, keyword arguments of NerfModel.workspace)
    ('infer', False): (False, {}), ('infer', True): (False, {'bf16': True}), ('infer', 'mlp'): (False, {'bf16': 'mlp'}),
    ('infer', 'x3'): (False, {'bf16': 'x3'}), ('infer', 'x3mlp'): (False, {'bf16': 'x3mlp'}),
    ('infer', 'jacobian'): (False, {'jacobian': True}),
    ('train', False): (True, {}), ('train', True): (True, {'bf16': True}), ('train', 'mlp'): (True, {'bf16': 'mlp'}),
    ('train', 'bg5+elastic'): (True, {'num_background_points': 5, 'elastic': True}),
    ('train', 'ray_grads'): (True, {'ray_grads': True}), ('train', 'ray_grads+elastic'): (True, {'ray_grads': True, 'elastic': True}),
}
PARENT_WORDS = {
    ('nowarp', 'infer', False): 2966720, ('nowarp', 'infer', True): 2966720, ('nowarp', 'infer', 'mlp'): 2966720,
    ('nowarp', 'infer', 'x3'): 3568832, ('nowarp', 'infer', 'x3mlp'): 3568832,
    ('nowarp', 'train', False): 20687424, ('nowarp', 'train', True): 28182336, ('nowarp', 'train', 'mlp'): 28182336,
    ('nowarp', 'train', 'ray_grads'): 23033216,
    ('warp', 'infer', False): 3276416, ('warp', 'infer', True): 3276416, ('warp', 'infer', 'mlp'): 3276416,
    ('warp', 'infer', 'x3'): 3929728, ('warp', 'infer', 'x3mlp'): 3929728, ('warp', 'infer', 'jacobian'): 5553920,
    ('warp', 'train', False): 23531392, ('warp', 'train', True): 27259392, ('warp', 'train', 'mlp'): 32255360,
    ('warp', 'train', 'bg5+elastic'): 26056576,
    ('warp', 'train', 'ray_grads'): 24996288, ('warp', 'train', 'ray_grads+elastic'): 26527488,
}


@pytest.mark.parametrize('kind', ['nowarp', 'warp'])
def test_workspace_sizes_are_the_parents(kind):
  model = _model(**(WARP if kind == 'warp' else {}))
  cases = [k for k in PARENT_WORDS if k[0] == kind]
  assert len(cases) == (12 if kind == 'warp' else 9)
  for case in cases:
    train, kw = _CALLS[case[1:]]
    assert model.workspace(B, train, 'cpu', **kw).numel() == PARENT_WORDS[case], case


def test_workspaces_are_shared_as_before():
  model = _model(**WARP)
  ws = lambda train, **kw: model.workspace(B, train, 'cpu', **kw)
  f32 = ws(False)
  assert ws(False) is f32 and ws(False, bf16=True) is f32 and ws(False, bf16='mlp') is f32   # only the TRAINING layout depends on bf16
  x3 = ws(False, bf16='x3')
  assert ws(False, bf16='x3mlp') is x3 and x3 is not f32
  assert ws(False, jacobian=True) is not f32
  train = [ws(True), ws(True, bf16=True), ws(True, bf16='mlp'), ws(True, ray_grads=True), ws(True, elastic=True),
           ws(True, num_background_points=5), ws(True, ray_grads=True, elastic=True)]
  assert len({t.data_ptr() for t in train + [f32, x3]}) == len(train) + 2   # one tensor per training mode, ray_grads its own
  assert ws(True, bf16='mlp') is train[2] and ws(True, ray_grads=True) is train[3]
  assert model.workspace(B + 1, False, 'cpu') is not f32


def test_one_flag_word():
  from nerfies_amd import lib as L
  model = _model(**WARP)
  assert model.flags() == 0
  assert model.flags(True, 'mlp', no_warp=True, jacobian=True, ray_grads=True) == (
      L.NRF_FLAG_TRAIN | L.NRF_FLAG_BF16 | L.NRF_FLAG_WARP_F32 | L.NRF_FLAG_NO_WARP | L.NRF_FLAG_WARP_JACOBIAN | L.NRF_FLAG_RAY_GRADS)
  for bf16 in (False, True, 'mlp', 'x3', 'x3mlp'):
    assert model.flags(bf16=bf16) == model.bf16_flags(bf16) and model.flags(True, bf16) == L.NRF_FLAG_TRAIN | model.bf16_flags(bf16)
  rec = model._record(B, model.flags(bf16='x3mlp', no_warp=True), 'cpu')   # the record keeps the call's word, not the sizing word
  assert rec.flags == L.NRF_FLAG_BF16X3 | L.NRF_FLAG_WARP_F32 | L.NRF_FLAG_NO_WARP and rec.num_rays == B
  assert rec.ws is model.workspace(B, False, 'cpu', bf16='x3') and rec.generation == model.generation
  assert rec[:2] == (B, rec.ws)   # indexes like the (B, ws) pair it replaced


def test_check_mode_raises_the_librarys_refusals():
  """Every mode on these models, against a direct nrf_workspace_bytes call with the word spelled out here: check_mode raises exactly
  where the library refuses, with the library's message."""
  import ctypes as C
  import re
  from nerfies_amd import lib as L
  bits = {False: 0, True: L.NRF_FLAG_BF16, 'mlp': L.NRF_FLAG_BF16 | L.NRF_FLAG_WARP_F32, 'x3': L.NRF_FLAG_BF16X3,
          'x3mlp': L.NRF_FLAG_BF16X3 | L.NRF_FLAG_WARP_F32}
  refused = set()
  for name, kw in (('plain', {}), ('warp', WARP), ('deep', {'nerf_rgb_branch_depth': 2}), ('deep+warp', dict(WARP, nerf_rgb_branch_depth=2))):
    model = _model(**kw)
    for train in (False, True):
      for bf16, word in bits.items():
        n = C.c_size_t(0)
        if model.lib.nrf_workspace_bytes(model.handle, 1, word | (L.NRF_FLAG_TRAIN if train else 0), C.byref(n)) == 0:
          model.check_mode(bf16, train=train)
          continue
        message = model.lib.nrf_last_error().decode()
        with pytest.raises(L.NrfError, match=re.escape(message)):
          model.check_mode(bf16, train=train)
        refused.add((name, train, bf16, 'NRF_FLAG_TRAIN' in message, 'nerf_rgb_branch_depth' in message))
  # the split-bf16 modes do not train; the bfloat16 chains have no second rgb branch layer
  assert {r[:3] for r in refused if r[3]} == {(m, True, b) for m in ('plain', 'warp', 'deep', 'deep+warp') for b in ('x3', 'x3mlp')}
  assert {r[:3] for r in refused if r[4]} == ({(m, False, b) for m in ('deep', 'deep+warp') for b in (True, 'mlp', 'x3', 'x3mlp')} |
                                             {(m, True, b) for m in ('deep', 'deep+warp') for b in (True, 'mlp')})
  assert all(r[3] or r[4] for r in refused)


def test_workspace_options_bump_the_generation_and_drop_everything():
  from nerfies_amd import models
  model = _model()
  g0 = model.generation   # 0, or 1 when NRF_CHAIN_TILE_ROWS set the option as the handle was made
  assert model.stash is None and model.last_call is None
  model.stash = models.CallRecord(B, model.workspace(B, True, 'cpu'), 1, model.generation)
  assert len(model._ws) == 1
  model.set_chain_tile_rows(32)
  assert model.generation == g0 + 1 and model._ws == {} and model.stash is None
  ws = model.workspace(B, True, 'cpu')
  model.stash = models.CallRecord(B, ws, 1, model.generation)
  model.set_chain_tile_rows(64)
  assert model.generation == g0 + 2 and model._ws == {} and model.stash is None
  assert model.workspace(B, True, 'cpu') is not ws
  # the same value again changes nothing in the library; the drop is unconditional, as it was before the generation existed
  model.set_chain_tile_rows(64)
  assert model.generation == g0 + 3 and model._ws == {}
  model.set_bf16_wgrad_merge(True)
  assert model.generation == g0 + 4


def test_backward_without_a_stash():
  from nerfies_amd import lib as L
  model = _model()
  rays = {'origins': torch.zeros(B, 3), 'directions': torch.ones(B, 3)}
  variables = {'params': None}   # not looked at before the refusal
  for args, kw in (((torch.ones(B, 3), torch.ones(B, 3)), {}), ((), {'d_out': {'fine': {'acc': torch.ones(B)}}}),
                   ((), {'ray_grads': True}), ((), {'d_out': {}, 'ray_grads': ('origins',)})):
    with pytest.raises(L.NrfError, match=r'backward\(\) needs a preceding apply\(\.\.\., train=True\)'):
      model.backward(variables, rays, *args, **kw)


def _recording_model(names, **cfg):
  """tests/helpers.py::cpu_field_model behind a RecordingLib for the entries `names`."""
  import helpers as H
  from nerfies_amd import lib as L
  rec = H.RecordingLib(L.load_library(), names)
  return (*H.cpu_field_model(rec, **cfg), rec)


@pytest.mark.parametrize('bad', ['shape', 'dtype', 'stride'])
def test_fused_steps_refuse_a_ray_gradient_output_they_cannot_write(bad):
  from nerfies_amd import lib as L
  model, fp, rec = _recording_model(['nrf_train_step_loss_grad_ex', 'nrf_train_step_loss_grad_rays', 'nrf_loss_grad_rays'],
                                    num_coarse_samples=8, num_fine_samples=6)
  batch = {'origins': torch.zeros(B, 3), 'directions': torch.ones(B, 3), 'rgb': torch.zeros(B, 3),
           'metadata': {'warp': torch.zeros(B, 1, dtype=torch.int32)}}
  out = {'shape': torch.zeros(B + 1, 3), 'dtype': torch.zeros(B, 3, dtype=torch.float64), 'stride': torch.zeros(3, B).t()}[bad]
  for step in (model.loss_and_grad, model.loss_and_ray_grads):
    with pytest.raises(L.NrfError, match=rf"{step.__name__}\(ray_grads_out=\.\.\.\): 'directions' .*\({B}, 3\)"):
      step(fp, batch, ray_grads=('origins', 'directions'), ray_grads_out={'directions': out})
  assert rec.calls == []


def test_workspace_options_drop_the_field_workspaces_with_the_rest(monkeypatch):
  import helpers as H
  model, fp, rec = _recording_model(['nrf_query_points', 'nrf_query_points_grad', 'nrf_unwarp_points'])
  H.lift_device_rule(monkeypatch)
  pts, ids = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32)
  keys = [('query', 1, 5, 'cpu'), ('query_grad', 1, 5, 'cpu'), ('unwarp', 5, 'cpu')]

  def run():
    """One call of each kind -> the workspace each ran in."""
    rec.calls.clear()
    model.query_points(fp, pts, metadata={'warp': ids[:1]}, outputs=('sigma',))
    model.query_gradient(fp, pts, metadata={'warp': ids[:1]}, outputs=('sigma',))
    model.unwarp_points(fp, pts, ids, None, outputs=('points',))
    assert [c['ws'] for c in rec.calls] == [model._ws[k].data_ptr() for k in keys] and len(model._ws) == 3
    return [c['ws'] for c in rec.calls]

  first = run()
  assert run() == first   # the cached ones, handed out again
  held, g0 = dict(model._ws), model.generation   # the old tensors stay alive here: a new one cannot be given one's address
  model.set_chain_tile_rows(32)
  assert model._ws == {} and model.generation == g0 + 1
  assert not set(run()) & set(first) and all(model._ws[k] is not held[k] for k in keys)
