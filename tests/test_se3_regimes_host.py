"""Rotation regimes on the CPU: helpers.rotation_regime places the SE3 heads' rotation angle where tests/test_gpu_se3_regimes.py needs
it, and every regime's conditions hold, on the float64 oracle, for the very cases (seeds, shapes) the GPU tests run -- so those
tests cannot drift out of their regime unnoticed."""
import pytest
import torch

import helpers as H

CASES = [(r, False) for r in H.ROTATION_REGIMES] + [('seam', True)]


@pytest.mark.parametrize('regime,three', CASES)
def test_regime_conditions_hold(regime, three):
  spec, B, tree, b64, stats = H.rotation_case(regime, three)
  H.assert_rotation_regime(regime, stats)
  for lv, s in stats.items():
    print(f'[{regime}{" 64+128" if three else ""} {lv}] rows {s["rows"]}: theta min {s["min"]:.3e} q10 {s["q10"]:.3e} median {s["median"]:.3e} '
          f'q90 {s["q90"]:.3e} max {s["max"]:.3e}; |v| median {s["v_median"]:.3e}; seam shares {s["seam_below"]:.2f} / {s["seam_above"]:.2f}; '
          f'below / above pi {s["below_pi"]:.2f} / {s["above_pi"]:.2f}')
  assert stats['coarse']['rows'] == B * spec.num_coarse_samples


def test_regime_touches_the_heads_only():
  spec, B, tree, b64, _ = H.rotation_case('seam')
  base = H.O.init_params(spec, seed=H.REGIME_SEED, trained_like=True, dtype=torch.float64)
  for (path, a), (_, b) in zip(H.O.tree_leaves_with_path(base), H.O.tree_leaves_with_path(tree)):
    same = torch.equal(a, b)
    assert same != ('branches_w' in path or 'branches_v' in path), path


def test_conditions_reject_the_stock_distribution():
  """The trained_like heads as they come are in none of the narrow regimes: the conditions are not vacuous."""
  spec, B, _, b64, _ = H.rotation_case('seam')
  base = H.O.init_params(spec, seed=H.REGIME_SEED, trained_like=True, dtype=torch.float64)
  stats = H.rotation_stats(H._warp_heads(base, spec, b64))
  for regime in ('init', 'tiny', 'seam', 'large'):
    with pytest.raises(AssertionError):
      H.assert_rotation_regime(regime, stats)
