"""Resources of dtqn_clip_adam_kernel from the build's remarks (libdtqn_hip.so.resources.json): no scratch, and the registers the
batched loads were allowed.  The parent kernel had 43 VGPRs; holding the thread's four float4s, its norm partial, the four status
words and the seven running statistics across the one barrier reaches 46."""
import json
import os

from dtqn_amd import build as dtqn_build

ADAM_VGPRS_MAX = 46


def test_clip_adam_kernel_has_no_scratch_and_46_vgprs_at_most():
    path = dtqn_build.resources_path()
    if not os.path.exists(path):
        dtqn_build.build()
    kernels = json.load(open(path))["kernels"]
    mine = [r for name, r in kernels.items() if "dtqn_clip_adam_kernel" in name]
    assert len(mine) == 1, sorted(kernels)
    assert mine[0]["scratch"] == 0, mine[0]
    assert mine[0]["vgprs"] <= ADAM_VGPRS_MAX, mine[0]
