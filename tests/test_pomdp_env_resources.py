"""Resources of the kernels the tabular POMDP environment kind changed, from the build's remarks (libdtqn_hip.so.resources.json): the
rollout's step and reset kernels and the evaluation's begin and step kernels still run without scratch -- the tables are read from
global memory through plain pointers, the binary search keeps no indexed private array -- and no kernel was added for the kind."""
import json
import os

from dtqn_amd import build as dtqn_build


def test_changed_rollout_and_evaluation_kernels_have_no_scratch():
    path = dtqn_build.resources_path()
    if not os.path.exists(path) or json.load(open(path)).get("src", "").split("+")[0] != dtqn_build._digest():
        dtqn_build.build()
    kernels = json.load(open(path))["kernels"]
    mine = {name: r for name, r in kernels.items() if "dtqn_rollout_" in name or "dtqn_deval_" in name}
    for want in ("dtqn_rollout_step_kernel", "dtqn_rollout_reset_kernel", "dtqn_rollout_commit_kernel", "dtqn_deval_begin_kernel",
                 "dtqn_deval_step_kernel"):
        assert sum(want in n for n in mine) == 1, (want, sorted(mine))
    assert len(mine) == 5, sorted(mine)
    for name, r in mine.items():
        assert r["scratch"] == 0 and r["lds"] == 0 and r["agprs"] == 0, (name, r)
        assert r["vgprs"] <= 128, (name, r)                           # one workgroup of DTQN_THREADS: no occupancy to protect, no spills either
