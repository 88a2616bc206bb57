"""Resources of the row-block embedding-gradient kernels: the panel kernel (tl_embed_bwd_panel_kernel) is in the resource table next to the
resident one, without scratch.  Their LDS is dynamic (dtqn_limits.h: dtqn_embed_bwd_lds / dtqn_embed_bwd_panel_lds), so the table holds no
byte count for it.  Compile-only (the table dtqn_amd.build keeps next to the library)."""
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


@pytest.mark.parametrize("name", ["tl_embed_bwd_panel_kernel", "tl_embed_bwd_kernel"])
def test_embedding_gradient_kernels_without_scratch(kernels, name):
    assert name in kernels, f"{name} missing from the resource table"
    r = kernels[name]
    assert r.get("scratch") == 0, (name, r)
    assert r.get("vgprs") is not None and r["vgprs"] <= 128, (name, r)       # 512 threads: two workgroups' worth of registers at most
