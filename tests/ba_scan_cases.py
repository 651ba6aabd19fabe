"""Case table of test_ba_multikernel_setup_gpu.py and of
oracle/make_ba_scan_golden.py: graphs sized at the boundaries of the integer
scans in the multi-kernel path's set-up (ba.hip ba_setup_kernel, 1024 threads).

Truncated graphs: the first n edges of cfg1 / cfg2 (one edge per patch there,
so n distinct patches): one edge, a wave boundary (63 / 64 / 65) and the
workgroup boundary (1023 / 1024 / 1025).
Wide kk range: cfg1 with its patch ids spread monotonically over a patch
buffer of `rows` rows.  33000 rows: the counting sort's histogram has more than
16384 bins, so its scan runs several chunks.  50000 rows: histogram + three
ints per edge exceed the 40832-int LDS budget and the bitonic fallback runs.
Every case: (graph, t0, t1, iterations)."""
import torch

from dpvo_amd import synthetic

SEED = 1  # the seed of test_ba_gpu.test_ba_matches_oracle
ITERS = 2


def _truncated(cfg, n):
    G = synthetic.make_config(cfg, seed=SEED)
    for k in ("ii", "jj", "kk", "target", "weight"):
        setattr(G, k, getattr(G, k)[:n].contiguous())
    return G, 1, G.F, ITERS


def _relabelled(rows):
    """cfg1 with patch k moved to row k * (rows - 1) // (F M - 1): the same
    problem, patch ids (and the kk range the set-up sorts over) spread out."""
    G = synthetic.make_config("cfg1", seed=SEED)
    n = G.F * G.M
    new = torch.arange(n, dtype=torch.int64) * (rows - 1) // (n - 1)
    patches = torch.zeros(rows, *G.patches.shape[1:])
    patches[:, 2] = 1.0
    patches[new] = G.patches[:n]
    G.patches = patches
    G.kk = new[G.kk].contiguous()
    return G, 1, G.F, ITERS


BA_SCAN_CASES = {}
for _n in (1, 2, 63, 64, 65):
    BA_SCAN_CASES[f"cfg1_first{_n}"] = (lambda n=_n: _truncated("cfg1", n))
for _n in (1023, 1024, 1025):
    BA_SCAN_CASES[f"cfg2_first{_n}"] = (lambda n=_n: _truncated("cfg2", n))
RELABELLED = ("cfg1_rows33000", "cfg1_rows50000")
BA_SCAN_CASES[RELABELLED[0]] = lambda: _relabelled(33000)
BA_SCAN_CASES[RELABELLED[1]] = lambda: _relabelled(50000)
