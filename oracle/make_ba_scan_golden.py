"""TEST INFRASTRUCTURE ONLY -- record what the multi-kernel BA path
(cuda_ba.select_path(2), ba.hip) returns for the cases of
tests/ba_scan_cases.py into tests/golden/ba_scan_parent.npz, for
tests/test_ba_multikernel_setup_gpu.py: `<case>__poses` (every pose) and
`<case>__depth` (the inverse depth of every touched patch, ascending patch id).

Needs a GPU.  Run it at the commit BEFORE a change that must keep that path's
bits (copy this script and tests/ba_scan_cases.py into that checkout); the
test then compares the changed tree with np.array_equal.

    python oracle/make_ba_scan_golden.py [--out tests/golden/ba_scan_parent.npz]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dpvo_amd  # noqa: E402
from ba_scan_cases import BA_SCAN_CASES  # noqa: E402


def run_case(cb, G, t0, t1, iters, dev):
    D = G.to(dev)
    poses, patches = D.poses.clone(), D.patches.clone()
    cb.forward(poses, patches, D.intrinsics, D.target, D.weight, torch.tensor([1e-4], device=dev),
               D.ii, D.jj, D.kk, G.M, t0, t1, iters, False)
    assert cb.check_status(poses) == 0
    touched = torch.unique(G.kk)
    return poses.cpu().numpy(), patches[touched.to(dev), 2, 0, 0].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "ba_scan_parent.npz"))
    args = ap.parse_args()
    cb = dpvo_amd.load_extension("cuda_ba")
    dev = torch.device("cuda:0")
    cb.check_status(torch.zeros(1, device=dev))  # clean slate
    cb.select_path(2)
    out = {}
    for name, make in BA_SCAN_CASES.items():
        G, t0, t1, iters = make()
        P, d = run_case(cb, G, t0, t1, iters, dev)
        again = run_case(cb, G, t0, t1, iters, dev)
        assert np.array_equal(P, again[0]) and np.array_equal(d, again[1]), name  # deterministic
        out[name + "__poses"], out[name + "__depth"] = P, d
        print(f"{name}: E={G.E} patches={d.size} N={t1 - t0} iterations={iters}", flush=True)
    cb.select_path(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
