"""Record what fastba.BA returns on the window path for the cases of
tests/ba_apply_cases.py into tests/golden/ba_apply_parent.npz: per case the
poses `<case>__poses`, the inverse depth of every patch `<case>__depths`
(patches[:, 2, 0, 0]; the BA writes the same value to all P * P elements of a
patch and never writes the x / y planes: asserted here, and the test checks
every element) and the last iteration's dX `<case>__dX` (fp64).

Run it on the GPU at the commit BEFORE a change that must keep the bits of the
BA window kernel's apply step (copy this script and tests/ba_apply_cases.py
into that checkout); test_ba_window_apply_gpu.py then compares the changed
tree with np.array_equal.

    python scripts/make_ba_apply_golden.py [--out tests/golden/ba_apply_parent.npz]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dpvo_amd  # noqa: E402,F401
import ba_apply_cases as C  # noqa: E402


def e_entries_in_hbm(G, t0, t1, iters, dev):
    """Whether workgroup 0 kept the E entries in the shared HBM buffer (mark 53)."""
    if t1 == t0:  # one workgroup, no E entries; the marks call needs a free pose
        return False, G.E
    cb = dpvo_amd.load_extension("cuda_ba")
    D = G.to(dev)
    m = cb.forward_marks(D.poses.clone(), D.patches.clone(), D.intrinsics, D.target, D.weight,
                         torch.tensor([1e-4], device=dev), D.ii, D.jj, D.kk, G.M, t0, t1, iters,
                         False).cpu().tolist()
    cb.check_status(D.poses)
    return int(m[53]) == 1, int(m[52])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "ba_apply_parent.npz"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for name, make in C.CASES.items():
        G, t0, t1, iters = make()
        P, K, dX, st = C.run(G, t0, t1, iters, dev)
        assert st == 0, (name, st)
        again = C.run(G, t0, t1, iters, dev)
        assert all(np.array_equal(a, b) for a, b in zip((P, K, dX), again[:3])), name  # deterministic
        assert np.isfinite(P).all() and np.isfinite(K).all() and np.isfinite(dX).all(), name
        assert np.array_equal(K[:, :2], G.patches.numpy()[:, :2]), name
        assert np.array_equal(K[:, 2], np.broadcast_to(K[:, 2, :1, :1], K[:, 2].shape)), name
        out[name + "__poses"], out[name + "__depths"], out[name + "__dX"] = P, K[:, 2, 0, 0], dX
        hbm, nrp = e_entries_in_hbm(G, t0, t1, iters, dev)
        d = K[:, 2, 0, 0]
        print(f"{name}: E={G.E} N={t1 - t0} P={K.shape[-1]} iterations={iters} workgroup 0: "
              f"{nrp} relevant edges, E entries {'in HBM' if hbm else 'in LDS'}; depths reset to 1: "
              f"{int((d == 1.0).sum())}, at the floor: {int((d == np.float32(1e-4)).sum())}",
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{len(C.CASES)} cases; wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
