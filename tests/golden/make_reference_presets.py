#!/usr/bin/env python
"""tests/golden/reference_presets.json: the configuration every preset of google/nerfies' configs/ resolves to, through its own
include chain, as nerfies_amd.gin_lite parses it -- each config dataclass as a dict, per preset file.  The presets themselves are
not copied; tests/test_configs_gin.py checks the shipped (flattened) presets and the preset checks against this record.

  python tests/golden/make_reference_presets.py PATH/TO/nerfies
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from nerfies_amd import configs  # noqa: E402
from nerfies_amd import gin_lite as gin  # noqa: E402

CLASSES = (configs.ExperimentConfig, configs.ModelConfig, configs.TrainConfig, configs.EvalConfig)
NOT_RUNNABLE = ('defaults.gin', 'warp_defaults.gin')   # "Do not run this directly": macros left for the includer


def effective(path):
  """Every config dataclass as a JSON-ready dict after parsing `path` from the current directory."""
  import dataclasses
  gin.clear_config()
  gin.parse_config_files_and_bindings([path], None, skip_unknown=True)
  out = {c.__name__: dataclasses.asdict(c()) for c in CLASSES}
  gin.clear_config()
  return json.loads(json.dumps(out))   # tuples -> lists, as the record holds them


def main(ref_root):
  old = os.getcwd()
  os.chdir(ref_root)            # the presets include both 'warp_defaults.gin' and 'configs/warp_defaults.gin'
  try:
    rec = {f: effective(os.path.join('configs', f)) for f in sorted(os.listdir('configs'))
           if f.endswith('.gin') and f not in NOT_RUNNABLE}
  finally:
    os.chdir(old)
  with open(os.path.join(HERE, 'reference_presets.json'), 'w') as fp:
    json.dump(rec, fp, indent=1, sort_keys=True)
    fp.write('\n')
  print('wrote', len(rec), 'presets')


if __name__ == '__main__':
  if len(sys.argv) != 2:
    raise SystemExit(__doc__)
  main(sys.argv[1])
