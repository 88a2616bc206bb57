"""Resources of the device-resident rollout's kernels from the build's remarks (libdtqn_hip.so.resources.json): every dtqn_rollout_
kernel runs without scratch -- the environment state, Memory's card tables and the staged episode live in global memory, no thread keeps
an indexed private array."""
import json
import os

from dtqn_amd import build as dtqn_build


def test_rollout_kernels_have_no_scratch():
    path = dtqn_build.resources_path()
    if not os.path.exists(path) or json.load(open(path)).get("src", "").split("+")[0] != dtqn_build._digest():
        dtqn_build.build()
    kernels = json.load(open(path))["kernels"]
    mine = {name: r for name, r in kernels.items() if "dtqn_rollout_" in name}
    assert len(mine) == 3 and any("dtqn_rollout_step_kernel" in n for n in mine), sorted(kernels)
    for name, r in mine.items():
        assert r["scratch"] == 0, (name, r)
