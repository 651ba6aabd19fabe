"""Record what the BA returns for the cases of tests/ba_setup_cases.py
(BA_CASES) into tests/golden/ba_setup_parent.npz: `<case>__poses` and
`<case>__patches`, the tensors cuda_ba.forward leaves behind.

Run it on the GPU at the commit BEFORE a change that must keep the BA's bits
(copy this script and tests/ba_setup_cases.py into that checkout); the test
test_ba_window_setup_gpu.py then compares the changed tree with
np.array_equal.

    python scripts/make_ba_setup_golden.py [--out tests/golden/ba_setup_parent.npz]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dpvo_amd  # noqa: E402
from ba_setup_cases import BA_CASES  # noqa: E402


def run_case(cb, G, t0, t1, iters, dev):
    D = G.to(dev)
    poses, patches = D.poses.clone(), D.patches.clone()
    cb.forward(poses, patches, D.intrinsics, D.target, D.weight, torch.tensor([1e-4], device=dev),
               D.ii, D.jj, D.kk, G.M, t0, t1, iters, False)
    assert cb.check_status(poses) == 0
    return poses.cpu().numpy(), patches.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "ba_setup_parent.npz"))
    args = ap.parse_args()
    cb = dpvo_amd.load_extension("cuda_ba")
    dev = torch.device("cuda:0")
    out = {}
    for name, make in BA_CASES.items():
        G, t0, t1, iters = make()
        P, K = run_case(cb, G, t0, t1, iters, dev)
        again = run_case(cb, G, t0, t1, iters, dev)
        assert np.array_equal(P, again[0]) and np.array_equal(K, again[1]), name  # deterministic
        out[name + "__poses"], out[name + "__patches"] = P, K
        print(f"{name}: E={G.E} N={t1 - t0} iterations={iters}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
