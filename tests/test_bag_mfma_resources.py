"""Resources of the matrix-core bag attention kernels (tl_bag_attn_mfma_kernel, tl_bag_attn_mfma_dq_kernel, tl_bag_attn_mfma_dkv_kernel):
every head width a bag network can have exists with and without dropout, without scratch, inside the 160 KB of LDS a workgroup can have
on gfx950.  Their LDS is static, so the figure in the table is the whole of it.  Compile-only (the table dtqn_amd.build keeps next to the
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
    out = {}
    for m, d in zip(mangled, names):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*\)$", "", d).replace("dtqn::", "")
        out[d] = data["kernels"][m]
    return out


@pytest.mark.parametrize("kind", ["tl_bag_attn_mfma_kernel", "tl_bag_attn_mfma_dq_kernel", "tl_bag_attn_mfma_dkv_kernel"])
@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("drop", ["false", "true"])
def test_matrix_core_bag_attention_instantiations(kernels, kind, hd, drop):
    name = f"{kind}<{hd}, {drop}>"
    assert name in kernels, f"{name} missing from the resource table"
    r = kernels[name]
    assert r.get("scratch") == 0, (name, r)
    lds = r.get("lds")
    assert lds is not None and 0 < lds < 160 * 1024, (name, r)
    # one 64-row block of two head-wide operands (+ 4 pad columns); the dk | dv kernel adds a 64 x 64 tile of weights and the delta row
    assert lds >= 64 * (2 * hd + 4) * 4, (name, r)
    # nothing grows with context x bag: the widest head stays under 96 KB
    assert lds <= 96 * 1024, (name, r)
