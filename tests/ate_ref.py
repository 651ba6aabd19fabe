"""Absolute trajectory error in fp64 numpy on the CPU: the comparison oracle of
test_ate_ref.py and test_evaluate_gpu.py.

Written from the contract in include/dpvo_hot.h: association by timestamp (the
rule of evo's sync.associate_trajectories as restated there: evo is not
available to check it against), Umeyama's Sim(3) alignment (np.linalg.svd,
umeyama_restatement.py) and plain numpy statistics.  The association is a
brute-force argmin over every stamp of the long side; it shares no code with
dpvo_amd/csrc/evaluate.hip (binary search, block scans, Jacobi SVD, radix
select).
"""
import numpy as np

from umeyama_restatement import umeyama_alignment


def is_sorted(t):
    t = np.asarray(t, np.float64)
    return bool(not np.isnan(t).any() and (t[:-1] <= t[1:]).all())


def associate(est_t, ref_t, max_diff=0.01):
    """-> int array [k, 2] of (est index, ref index), in short-side order."""
    est_t = np.asarray(est_t, np.float64)
    ref_t = np.asarray(ref_t, np.float64)
    est_long = len(est_t) > len(ref_t)
    long_t, short_t = (est_t, ref_t) if est_long else (ref_t, est_t)
    pairs = []
    for s, ts in enumerate(short_t):
        dt = np.abs(long_t - ts)
        l = int(np.argmin(dt))  # the first of equal minima: ties go to the lower index
        if dt[l] <= max_diff:
            pairs.append((l, s) if est_long else (s, l))
    return np.asarray(pairs, np.int64).reshape(-1, 2)


def ate(est_xyz, est_t, ref_xyz, ref_t, max_diff=0.01, align=True):
    """dict(stats [8] = rmse mean median std min max sse count, model [13] =
    R t c, pairs [min(n, m), 2] (unused rows -1), status, errors)."""
    est_xyz = np.asarray(est_xyz, np.float64)[:, :3]
    ref_xyz = np.asarray(ref_xyz, np.float64)[:, :3]
    n, m = len(est_xyz), len(ref_xyz)
    status = 0
    if is_sorted(est_t) and is_sorted(ref_t):
        p = associate(est_t, ref_t, max_diff)
    else:
        status |= 4
        p = np.zeros((0, 2), np.int64)
    k = len(p)
    pairs = np.full((min(n, m), 2), -1, np.int64)
    pairs[:k] = p
    if k < 3:
        status |= 1
    R, t, c = np.eye(3), np.zeros(3), 1.0
    x, y = est_xyz[p[:, 0]], ref_xyz[p[:, 1]]
    if status == 0 and align:
        fit = umeyama_alignment(x, y)
        if fit is None:
            status |= 2
        else:
            R, t, c = fit
    stats = np.full(8, np.nan)
    stats[7] = k
    e = np.zeros(0)
    if status == 0:
        e = np.sqrt((((c * x @ R.T) + t - y) ** 2).sum(1))
        stats[:7] = [np.sqrt((e * e).mean()), e.mean(), np.median(e), e.std(), e.min(), e.max(),
                     (e * e).sum()]
    return dict(stats=stats, model=np.concatenate([R.reshape(-1), t, [c]]), pairs=pairs,
                status=status, errors=e)


def make_case(n, m, seed, max_diff=0.01, noise=1e-2, drop=3, dtype=np.float64):
    """A ground-truth curve of extent <= 10 sampled at m stamps, an estimate at n
    stamps that is the curve moved by a Sim(3) plus noise.  Stamps of the short
    side sit on stamps of the long side, jittered by at most max_diff / 2;
    `drop` of them are pushed beyond max_diff.  -> est_xyz, est_t, ref_xyz, ref_t."""
    from umeyama_restatement import rotation_of

    g = np.random.default_rng(seed)
    nl, ns = max(n, m), min(n, m)
    # spacing >= 0.04: a stamp pushed 1.2 .. 2.2 max_diff off its partner reaches no other one
    long_t = 100.0 + 0.05 * np.arange(nl) + g.uniform(-0.005, 0.005, nl)
    long_t.sort()
    pick = np.sort(g.choice(nl, ns, replace=False))
    short_t = long_t[pick] + g.uniform(-0.5, 0.5, ns) * max_diff
    for i in g.choice(ns, min(drop, ns), replace=False):
        short_t[i] += 1.7 * max_diff
    short_t.sort()

    def curve(t):
        s = (t - 100.0) / (0.05 * nl)
        return np.stack([4.5 * np.cos(5 * s), 4.5 * np.sin(3 * s), 2.0 * s + np.sin(7 * s)], 1)

    est_t, ref_t = (long_t, short_t) if n > m else (short_t, long_t)
    ref_xyz = curve(ref_t)
    R, t, c = rotation_of([0.4, -0.2, 0.7]), np.array([0.5, -0.3, 0.8]), 1.3
    # est = the inverse Sim(3) of the truth, so that ref ~ c R est + t; extent stays <= 10
    est_xyz = ((curve(est_t) - t) @ R) / c + noise * g.standard_normal((n, 3))
    return est_xyz.astype(dtype), est_t, ref_xyz, ref_t
