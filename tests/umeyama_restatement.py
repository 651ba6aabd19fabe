"""Umeyama alignment and its RANSAC loop in fp64 numpy on the CPU: the
comparison oracle of the loop-closure measurement tests
(test_umeyama_restatement.py, test_ransac_umeyama_gpu.py, test_close_loop_gpu.py).

Written from the algorithm (Umeyama, "Least-squares estimation of
transformation parameters between two point patterns", PAMI 1991, eq. 34-43)
with np.linalg.svd; the loop is the sequential RANSAC of
dpvo/loop_closure/optim_utils.py:117-150 with the samples passed in and the
early-exit count as a parameter.  It shares no code with the kernels of
dpvo_amd/csrc/ransac.hip (which use a one-sided Jacobi SVD completed by cross
products and pick the winner from all counts at once).
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def umeyama_alignment(x, y):
    """x, y [n, 3] -> (R, t, c) with y ~ c R x + t, or None when fewer than
    two singular values of the covariance exceed eps (absolute)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n = x.shape[0]
    mean_x = x.sum(0) / n
    mean_y = y.sum(0) / n
    xc, yc = x - mean_x, y - mean_y
    sigma_x = (xc * xc).sum() / n                      # eq. 36
    cov = yc.T @ xc / n                                # eq. 38
    u, d, vt = np.linalg.svd(cov)
    if np.count_nonzero(d > EPS) < 2:
        return None
    s = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:     # eq. 43
        s[2, 2] = -1.0
    R = u @ s @ vt                                     # eq. 40
    c = np.trace(np.diag(d) @ s) / sigma_x             # eq. 42
    t = mean_y - c * (R @ mean_x)                      # eq. 41
    return R, t, c


def distances(model, src, dst):
    R, t, c = model
    return np.sqrt((((src @ (c * R).T) + t - dst) ** 2).sum(1))


def ransac_umeyama(src, dst, samples, threshold=0.1, early_exit=100):
    """The sequential loop over samples [H, 3].  Returns a dict: R, t, s (None
    when there is no model), num_inliers, winner (-1: none), stop (the index of
    the last hypothesis looked at), mask [N] of the winner, counts [H] of
    EVERY hypothesis (-1: degenerate sample; the loop itself only looks at
    counts[:stop + 1]), min_margin = min |distance - threshold| over all
    (hypothesis, point), and status (0 ok, 1 no positive count, 2 the refit
    on the winner's inliers is degenerate)."""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    H, N = len(samples), len(src)
    counts = np.full(H, -1, np.int64)
    masks = np.zeros((H, N), bool)
    margin = np.inf
    for h in range(H):
        idx = np.asarray(samples[h])
        model = umeyama_alignment(src[idx], dst[idx])
        if model is None:
            continue
        dist = distances(model, src, dst)
        masks[h] = dist < threshold
        counts[h] = masks[h].sum()
        margin = min(margin, np.abs(dist - threshold).min())
    best, winner, stop = 0, -1, H - 1
    for h in range(H):
        if counts[h] < 0:
            continue
        if counts[h] > best:
            best, winner = int(counts[h]), h
        if counts[h] > early_exit:
            stop = h
            break
    out = dict(R=None, t=None, s=None, num_inliers=best, winner=winner, stop=stop,
               mask=masks[winner].copy() if winner >= 0 else np.zeros(N, bool), counts=counts,
               min_margin=margin, status=1)
    if winner >= 0:
        fit = umeyama_alignment(src[out["mask"]], dst[out["mask"]])
        out["status"] = 2 if fit is None else 0
        if fit is not None:
            out["R"], out["t"], out["s"] = fit
    return out


def rotation_of(rotvec):
    """Rodrigues' formula."""
    rotvec = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(rotvec)
    k = rotvec / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def quaternion_of(R):
    """(x, y, z, w) with w >= 0 from the eigenvector of the 4x4 K matrix of R
    (Bar-Itzhack 2000): no branch on the trace."""
    K = np.array([
        [R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
        [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
        [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
        [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]],
    ]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[:, np.argmax(w)]
    return q if q[3] >= 0 else -q


TRUTH = (rotation_of([0.3, -0.5, 0.8]), np.array([0.4, -1.1, 2.0]), 1.7)

# (N, H, seed, outlier_frac) -> (stop, winner, inliers) as found on the CPU
CASES = {
    (257, 64, 7, 0.4): (3, 3, 161),
    (90, 64, 8, 0.4): (63, 5, 55),
    (90, 400, 9, 0.5): (399, 57, 36),
    (2048, 400, 10, 0.6): (5, 5, 813),
    (33, 64, 11, 0.3): (63, 0, 24),
}


def make_case(N, H, seed, outlier_frac, noise=0.01):
    """(src [N, 3], dst [N, 3], samples [H, 3] int64), fp64."""
    g = np.random.default_rng(seed)
    src = g.uniform(-2, 2, (N, 3))
    src[:, 2] = g.uniform(1, 8, N)
    R, t, s = TRUTH
    dst = s * src @ R.T + t + noise * g.standard_normal((N, 3))
    out = g.random(N) < outlier_frac
    dst[out] = g.uniform(-10, 10, (int(out.sum()), 3))
    samples = np.stack([g.choice(N, 3, replace=False) for _ in range(H)])
    return src, dst, samples
