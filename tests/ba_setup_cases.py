"""Case tables of the BA window set-up tests (test_ba_window_setup_gpu.py,
test_ba_window_setup_cases.py) and of scripts/make_ba_setup_golden.py, plus a
host restatement of the pose-slot function the plan stores per sorted position.

Pose slots (ba_window.hip wslot): the window kernel keeps a table of 64 poses
in LDS, the N free poses [t0, t0 + N) first, then the fixed poses from fmin
(the smallest fixed pose any edge touches) upward; a fixed pose past the table
gets 0xFE ("read it from HBM").  pslot[p] = slot(ii[e]) | slot(jj[e]) << 8 for
the edge e at sorted position p (edges grouped by patch id, ascending edge
index inside a patch)."""
import numpy as np

K_SLOTS = 64
K_HBM = 0xFE
INT_MAX = 2 ** 31 - 1
META_BYTES = 4 * (64 + 16 * 136)  # the plan meta block; pslot lies right behind it


def wslot(gp, t0, N, fmin):
    gp = np.asarray(gp, np.int64)
    k = gp - fmin
    fixed = np.where((k >= 0) & (k < K_SLOTS - N), N + k, K_HBM)
    return np.where((gp >= t0) & (gp < t0 + N), gp - t0, fixed).astype(np.int64)


def fmin_of(ii, jj, t0, t1, num_poses):
    both = np.concatenate([ii, jj])
    fixed = both[(both < t0) | (both >= t1)]
    return int(np.clip(fixed, 0, num_poses - 1).min()) if fixed.size else INT_MAX


def pslot_ref(ii, jj, kk, t0, t1, num_poses):
    """(pslot by sorted position, fmin) as the plan must write them."""
    fmin = fmin_of(ii, jj, t0, t1, num_poses)
    order = np.argsort(kk, kind="stable")
    N = t1 - t0
    ps = wslot(ii[order], t0, N, fmin) | (wslot(jj[order], t0, N, fmin) << 8)
    return ps.astype(np.uint16), fmin


def patch_masks(ii, jj, kk, t0, t1):
    """Free-pose bitmask of every distinct patch (ascending patch id)."""
    bits = np.zeros(kk.size, np.int64)
    for x in (ii, jj):
        free = (x >= t0) & (x < t1)
        bits |= np.where(free, 1 << np.clip(x - t0, 0, 31), 0)
    uk, inv = np.unique(kk, return_inverse=True)
    m = np.zeros(uk.size, np.int64)
    np.bitwise_or.at(m, inv, bits)
    return m


# ---- graphs for the pslot check: (ii, jj, kk, M, num_poses, (t0, t1)) ----
def _random(E, nk, M, F, window, seed):
    rng = np.random.default_rng(seed)
    base = np.sort(rng.choice(F * M, nk, replace=False))
    kk = rng.permutation(np.concatenate([base, base[rng.integers(0, nk, E - nk)]]))
    return (np.ascontiguousarray(kk // M, np.int64), rng.integers(0, F, E).astype(np.int64),
            np.ascontiguousarray(kk, np.int64), M, F, window)


PSLOT_CASES = {
    "E96_40patches": lambda: _random(96, 40, 96, 12, (1, 12), 10),
    "E700_650patches": lambda: _random(700, 650, 96, 12, (1, 12), 11),
    # patch ids spread over 12 * 2048: wider than the counting sort's range (bitonic path)
    "E2048_1500patches_M2048": lambda: _random(2048, 1500, 2048, 12, (1, 12), 12),
    # 90 fixed poses below a window of 10: those past slot 63 are read from HBM
    "hbm_fixed_poses": lambda: _random(1200, 500, 16, 100, (90, 100), 13),
    # every pose free: fmin stays INT_MAX
    "no_fixed_pose": lambda: _random(600, 300, 96, 12, (0, 12), 14),
}
PSLOT_DEVICE_T0 = "E700_650patches"  # also planned with t0 as a device scalar


# ---- graphs for the BA check: name -> (Graph, t0, t1, iterations) ----
def _graph(**kw):
    """Lateral motion (parallax) and 0.05 px of target noise: at the defaults
    (0.5 px, none) the first depth update of some patches runs into the clamps."""
    from dpvo_amd import synthetic

    return synthetic.make_graph(noise=0.05, lateral=0.05, **kw)


def _dpvo(iters):
    from dpvo_amd import synthetic

    G = synthetic.make_dpvo_window(n=10, seed=3)
    return G, max(G.F - 10, 1), G.F, iters  # dpvo.py:818-824: t0 = max(n - 10, 1)


BA_CASES = {
    "N0": lambda: (_graph(F=18, M=8, E=300, seed=30), 1, 1, 2),
    "N1": lambda: (_graph(F=18, M=8, E=300, seed=31), 1, 2, 2),
    "N2": lambda: (_graph(F=18, M=8, E=300, seed=32), 1, 3, 2),
    "N11": lambda: (_graph(F=18, M=8, E=300, seed=33), 1, 12, 2),
    "N16": lambda: (_graph(F=18, M=8, E=300, seed=34), 1, 17, 2),
    # window in the middle: the patches of the first frames see no free pose
    "no_free_pose_patches": lambda: (_graph(F=18, M=8, E=300, seed=35), 9, 11, 2),
    # 2304 distinct patches: the second batch of plan entries
    "nuniq_gt_2048": lambda: (_graph(F=24, M=96, E=2400, seed=30), 1, 9, 2),
    "E2048": lambda: (_graph(F=12, M=96, E=2048, seed=40), 1, 12, 2),  # cfg2's shape
    "E2049": lambda: (_graph(F=12, M=96, E=2049, seed=37), 1, 12, 2),
    "E8": lambda: (_graph(F=4, M=2, E=8, seed=38), 1, 4, 2),
    # fixed poses past the LDS pose table on edges into the window
    "hbm_fixed_poses": lambda: (_graph(F=80, M=4, E=400, seed=39), 70, 80, 2),
    "dpvo_n10_it1": lambda: _dpvo(1),
    "dpvo_n10_it2": lambda: _dpvo(2),
}
