"""Records tests/golden/devenv_parent_bits.npz: the scenarios of tests/devenv_bits_helpers.py, run at the commit BEFORE the shared
device-environment layer.  Never re-record it from a later commit: the file is what that refactor is held against.

    python tests/golden/make_devenv_parent_bits.py --device cuda --out gpu.npz                    (the MI355X: epsilon = 1, rollout only)
    python tests/golden/make_devenv_parent_bits.py --device cpu --gpu-recording gpu.npz --out tests/golden/devenv_parent_bits.npz
    python tests/golden/make_devenv_parent_bits.py --compare <a.npz> <b.npz>                      (same keys, same bytes?)

It prints a sha1 per array; two emulation runs in separate processes gave equal files (the scenario is deterministic).  An array of
the MI355X recording that differs from the emulation's is kept under "gpu/<key>", the others once.  At the parent one did:
car/eps1/rollout_state, in the last bit of the f64 position of two of the three episodes in progress (CarFlag.reset's -0.2 + 0.4 u,
which they start from, is one fused multiply-add on the GPU and two roundings on the host; the f32 observations agree)."""
import argparse
import hashlib
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]


def record(device, out, gpu_recording=None):
    import devenv_bits_helpers as H
    if device == "cpu":
        from dtqn_amd import _binding as B
        from emu import emu_build
        lib = B.load_library(emu_build.build())
    else:
        from dtqn_amd import engine
        engine.require_gpu()
        lib = None
    arrays = {}
    for kind in H.KINDS:
        for eps_name, eps in H.EPSILONS.items():
            if device != "cpu" and eps < 1.0:
                continue
            got = H.run_scenario(lib, device, kind, eps, with_eval=device == "cpu")
            for name, a in got.items():
                arrays[f"{kind}/{eps_name}/{name}"] = a
    if gpu_recording:
        z = np.load(gpu_recording)
        for key in z.files:
            if z[key].dtype != arrays[key].dtype or z[key].tobytes() != arrays[key].tobytes():
                arrays["gpu/" + key] = z[key]
    for key in sorted(arrays):
        print(key, arrays[key].dtype, arrays[key].shape, hashlib.sha1(arrays[key].tobytes()).hexdigest())
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


def compare(a, b):
    za, zb = np.load(a), np.load(b)
    common = sorted(set(za.files) & set(zb.files))
    bad = [k for k in common if za[k].dtype != zb[k].dtype or za[k].tobytes() != zb[k].tobytes()]
    print(len(common), "common arrays,", len(bad), "differ:", bad)
    return 1 if bad or not common else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    ap.add_argument("--out")
    ap.add_argument("--gpu-recording")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    record(args.device, args.out, args.gpu_recording)
