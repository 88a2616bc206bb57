"""Resources of the one-launch weight-gradient kernel (dtqn_wgrad_direct_kernel): the batched kernel-argument fetch of round 7 keeps it
without scratch and at or below the 109 vector registers it had before (1024 threads per workgroup: four waves per SIMD whatever the
count, but every register beside the walk is one less for the operands in flight).  Compile-only (the table dtqn_amd.build keeps next to
the library)."""
import json
import os
import re
import subprocess

import pytest

from dtqn_amd import build as B


@pytest.fixture(scope="module")
def kernels():
    path = B.resources_path()
    stale = True
    if os.path.exists(path):
        with open(path) as f:
            stale = json.load(f).get("src", "").split("+")[0] != B._digest()
    if stale:
        B.build()
    with open(path) as f:
        data = json.load(f)
    assert data["src"].split("+")[0] == B._digest(), "resource table does not belong to this source tree"
    mangled = sorted(data["kernels"])
    names = subprocess.run(["c++filt"] + mangled, capture_output=True, text=True, check=True).stdout.splitlines()
    out = {}
    for m, d in zip(mangled, names):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*\)$", "", d).replace("dtqn::", "")
        out[d] = data["kernels"][m]
    return out


def test_direct_weight_gradient_kernel_registers_and_scratch(kernels):
    name = "dtqn_wgrad_direct_kernel"
    assert name in kernels, f"{name} missing from the resource table"
    r = kernels[name]
    assert r.get("scratch") == 0, (name, r)
    assert r.get("vgprs") is not None and r["vgprs"] <= 109, (name, r)
    assert r.get("agprs", 0) == 0, (name, r)
