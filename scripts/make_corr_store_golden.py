"""Record what A-CORR returns for the cases of tests/corr_store_cases.py into
tests/golden/corr_store_parent.npz: per (shape, feature dtype, level set) the
output [1, E, Dp, Dp, p, p, L] of the unordered launch at the largest edge
count.  Every other case of the table (fewer edges, the XCD order) is run too
and must equal a prefix of that array bit for bit, so the one array is the
fixture of all of them.

Run it on the GPU at the commit BEFORE a change that must keep A-CORR's bits
(copy this script, tests/corr_store_cases.py into that checkout);
test_corr_store_paths_gpu.py then compares the changed tree with np.array_equal.

    python scripts/make_corr_store_golden.py [--out tests/golden/corr_store_parent.npz]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dpvo_amd  # noqa: E402,F401
import corr_store_cases as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "corr_store_parent.npz"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = S.cases()
    out = {}
    # the widest unordered case of every key first
    for c in sorted(cases, key=lambda c: (-c["E"], c["ordered"])):
        k = S.key(c["shape"], c["dname"], c["levels"], c["bad"])
        a, again, _ = S.run(dev, c)
        assert np.isfinite(a).all() and np.array_equal(a, again), S.case_id(c)
        if k not in out:
            assert not c["ordered"]
            out[k] = a
        assert np.array_equal(a, out[k][:, :c["E"]]), S.case_id(c)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{len(cases)} cases, {len(out)} arrays; wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
