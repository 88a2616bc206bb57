"""Resources of the device-resident bags' kernels from the build's remarks (libdtqn_hip.so.resources.json): the two dtqn_devbag_ kernels
run without scratch -- bags, candidates and scores live in global memory and LDS, no thread keeps an indexed private array."""
import json
import os

from dtqn_amd import build as dtqn_build
from dtqn_amd.agents import device_bag  # noqa: F401  (the feature these kernels serve)


def test_devbag_kernels_have_no_scratch():
    path = dtqn_build.resources_path()
    if not os.path.exists(path) or json.load(open(path)).get("src", "").split("+")[0] != dtqn_build._digest():
        dtqn_build.build()
    kernels = json.load(open(path))["kernels"]
    mine = {name: r for name, r in kernels.items() if "dtqn_devbag_" in name}
    assert len(mine) == 2, sorted(kernels)
    assert any("dtqn_devbag_stage_kernel" in n for n in mine) and any("dtqn_devbag_select_kernel" in n for n in mine), sorted(mine)
    for name, r in mine.items():
        assert r["scratch"] == 0, (name, r)
    assert not any("dtqn_rollout_" in n or "dtqn_deval_" in n for n in mine)
