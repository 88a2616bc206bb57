"""Resources of the kernels of the greedy evaluation (dtqn_actor.hip: live-context compaction, Q rows + arg-max): present in the table
dtqn_amd.build keeps next to the library, without scratch.  Compile-only."""
import json
import os
import re
import subprocess

import pytest

from dtqn_amd import build as B

KERNELS = ("actor_compact_kernel", "actor_greedy_kernel")


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


@pytest.mark.parametrize("name", KERNELS)
def test_greedy_kernels_use_no_scratch(kernels, name):
    assert name in kernels, f"{name} missing from the resource table"
    r = kernels[name]
    assert r.get("source") == "dtqn_actor.hip" and r.get("scratch") == 0, (name, r)
    assert r.get("lds") == 1024, (name, r)          # the live count / scan: one int per thread of the workgroup
