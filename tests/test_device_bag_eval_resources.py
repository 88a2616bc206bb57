"""Resources of what the device-resident evaluation of a bag network adds, from the build's remarks (libdtqn_hip.so.resources.json): the
broadcast of the shared-trunk candidate forward (tl_bcast_kernel) runs without scratch, and the feature added no kernel under the names
the bags' and the evaluation's resource tests count."""
import json
import os

from dtqn_amd import build as dtqn_build
from dtqn_amd.agents import device_bag_eval  # noqa: F401  (the feature these kernels serve)


def test_added_kernels_have_no_scratch_and_the_pinned_counts_stay():
    path = dtqn_build.resources_path()
    if not os.path.exists(path) or json.load(open(path)).get("src", "").split("+")[0] != dtqn_build._digest():
        dtqn_build.build()
    kernels = json.load(open(path))["kernels"]
    mine = {name: r for name, r in kernels.items() if "tl_bcast_kernel" in name}
    assert len(mine) == 1, sorted(kernels)
    for name, r in mine.items():
        assert r["scratch"] == 0, (name, r)
    assert len([n for n in kernels if "dtqn_devbag_" in n]) == 2 and len([n for n in kernels if "dtqn_deval_" in n]) == 2, sorted(kernels)
