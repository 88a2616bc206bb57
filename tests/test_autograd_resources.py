"""Resources of the kernels the differentiable forward added (tl_dq_in_kernel: the caller's dL/dQ into the records; tl_dobs_kernel: the
observation gradient) and of the embedding backward it extended: no scratch, no LDS of their own.  Compile-only (the table dtqn_amd.build
keeps next to the library)."""
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
    return {re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", d)).replace("dtqn::", ""): data["kernels"][m] for m, d in zip(mangled, names)}


@pytest.mark.parametrize("name", ["tl_dq_in_kernel", "tl_dobs_kernel", "tl_embed_bwd_kernel"])
def test_autograd_kernels_without_scratch(kernels, name):
    assert name in kernels, f"{name} missing from the resource table"
    r = kernels[name]
    assert r.get("scratch") == 0, (name, r)
    if name != "tl_embed_bwd_kernel":
        assert r.get("lds", 0) == 0, (name, r)
