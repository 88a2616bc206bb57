"""Resources of the device-resident evaluation's kernels from the build's remarks (libdtqn_hip.so.resources.json): exactly the two
dtqn_deval_ kernels exist and both run without scratch -- the environment state and the results table live in global memory, no
thread keeps an indexed private array."""
import json
import os

from dtqn_amd import build as dtqn_build


def test_deval_kernels_have_no_scratch():
    path = dtqn_build.resources_path()
    if not os.path.exists(path) or json.load(open(path)).get("src", "").split("+")[0] != dtqn_build._digest():
        dtqn_build.build()
    kernels = json.load(open(path))["kernels"]
    mine = {name: r for name, r in kernels.items() if "dtqn_deval_" in name}
    assert len(mine) == 2, sorted(kernels)
    assert any("dtqn_deval_begin_kernel" in n for n in mine) and any("dtqn_deval_step_kernel" in n for n in mine), sorted(mine)
    for name, r in mine.items():
        assert r["scratch"] == 0, (name, r)
