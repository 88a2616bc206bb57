"""Resources of the attention-capture kernels (tl_alpha_kernel at every head width of the row-block path, tl_bag_alpha_kernel): no
scratch, LDS inside the 160 KB a workgroup can have on gfx950 (static, so the table's figure is the whole of it).  The kernel is not
templated on d_model, so these instantiations serve D = 64 / 128 / 256 alike.  Compile-only (the table dtqn_amd.build keeps next to the
library)."""
import json
import os
import re
import subprocess

import pytest

from dtqn_amd import build as B

HEAD_DIMS = (4, 8, 16, 32, 64, 128)


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


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_alpha_kernel_instantiations(kernels, hd):
    name = f"tl_alpha_kernel<{hd}>"
    assert name in kernels, f"{name} missing from the resource table"
    r = kernels[name]
    assert r.get("scratch") == 0, (name, r)
    lds = r.get("lds")
    # one 64-row key block of the head (+ 4 pad columns), reused as the 64 x 65 output tile
    assert lds is not None and max(64 * (hd + 4), 64 * 65) * 4 <= lds <= 160 * 1024, (name, r)


def test_bag_alpha_kernel(kernels):
    r = kernels.get("tl_bag_alpha_kernel")
    assert r is not None and r.get("scratch") == 0 and r.get("lds", 0) == 0, r
