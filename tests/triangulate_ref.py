"""numpy restatement (fp64) of dpvo_amd.long_term.triangulate_tracks
(csrc/triangulate.hip) and the synthetic frame triplet its tests share.

The restatement follows the kernel step by step: lower median, `iterations`
steps dZ = u / (C + lmbda) over the two observations with the reference's
linearisation and gates (ba_cuda.cu:265-333), the retraction clamp
(:225-228), the reprojection residuals, the un-projection and the keep rule."""
from types import SimpleNamespace

import numpy as np

# (fx, fy, cx, cy) at image resolution, as tests/test_tracker_gpu.py
K_IMAGE = np.array([320.0, 320.0, 48.0, 32.0])
HT, WD = 64, 96


def quat_to_R(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def relative(pi, pj):
    """(R_ij, t_ij) of Gj Gi^-1 for poses (t, q xyzw), X_cam = R X_world + t."""
    Ri, Rj = quat_to_R(pi[3:]), quat_to_R(pj[3:])
    Rij = Rj @ Ri.T
    return Rij, pj[:3] - Rij @ pi[:3]


def project(Rij, tij, K, uv, d):
    """Pixels of frame-i keypoints uv [n, 2] at inverse depth d [n] in frame j
    -> (pixels [n, 2], X, Y, Z)."""
    fx, fy, cx, cy = K
    X0 = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], 1)
    Xj = X0 @ Rij.T + d[:, None] * tij[None]
    return np.stack([fx * Xj[:, 0] / Xj[:, 2] + cx, fy * Xj[:, 1] / Xj[:, 2] + cy], 1), Xj


def lower_median(v):
    return np.sort(np.asarray(v))[(len(v) - 1) // 2]


def triangulate_ref(poses, intrinsics, disps, kps0, kps1, kps2, m10, m12, max_depth=20.0,
                    max_residual=2.0, iterations=6, lmbda=1e-3):
    f = np.float64
    poses, intrinsics = np.asarray(poses, f), np.asarray(intrinsics, f)
    kps = [np.asarray(k, f) for k in (kps0, kps1, kps2)]
    N1 = len(kps[1])
    track = (m10 >= 0) & (m10 < len(kps[0])) & (m12 >= 0) & (m12 < len(kps[2]))
    tr = np.nonzero(track)[0]
    K = intrinsics[0]  # the BA and the reprojection read row 0
    fx, fy, cx, cy = K
    uv = kps[1][tr]
    tgt = [kps[0][m10[tr]], kps[2][m12[tr]]]
    rel = [relative(poses[1], poses[0]), relative(poses[1], poses[2])]
    d = np.full(len(tr), f(np.float32(lower_median(disps))))
    lam = f(np.float32(lmbda))

    def linearise(o, d):
        Rij, tij = rel[o]
        px, Xj = project(Rij, tij, K, uv, d)
        X, Y, Z = Xj.T
        r = tgt[o] - px
        iz = np.where(Z >= 0.2, 1.0 / Z, 0.0)
        ok = ((np.hypot(r[:, 0], r[:, 1]) < 128) & (Z > 0.2) & (px[:, 0] > -64) & (px[:, 1] > -64)
              & (px[:, 0] < 2 * cx + 64) & (px[:, 1] < 2 * cy + 64))
        Jz = np.stack([fx * (tij[0] * iz - tij[2] * X * iz * iz),
                       fy * (tij[1] * iz - tij[2] * Y * iz * iz)], 1)
        return ok.astype(f), r, Jz

    for _ in range(iterations):
        C, U = np.zeros(len(tr)), np.zeros(len(tr))
        for o in range(2):
            w, r, Jz = linearise(o, d)
            C += w * (Jz * Jz).sum(1)
            U += w * (r * Jz).sum(1)
        d = d + U / (C + lam)
        d = np.where(d > 20.0, 1.0, d)
        d = np.maximum(d, 1e-4)
    res = np.zeros(len(tr))
    for o in range(2):
        _, r, _ = linearise(o, d)
        res = np.maximum(res, np.hypot(r[:, 0], r[:, 1]))
    Ki = intrinsics[1]
    pts = np.stack([(uv[:, 0] - Ki[2]) / Ki[0], (uv[:, 1] - Ki[3]) / Ki[1], np.ones(len(tr))], 1)
    pts = pts / d[:, None]
    out = SimpleNamespace(points=np.zeros((N1, 3)), disp=np.zeros(N1), keep=np.zeros(N1, bool),
                          residual=np.full(N1, np.inf), track=track)
    out.points[tr], out.disp[tr], out.residual[tr] = pts, d, res
    out.keep[tr] = (res < max_residual) & (pts[:, 2] < max_depth)
    kept = np.nonzero(out.keep)[0]
    out.sel = np.full(N1, -1, np.int64)
    out.sel[:len(kept)] = kept
    out.count = len(kept)
    return out


def _quat(axis_angle):
    a = np.asarray(axis_angle, np.float64)
    th = np.linalg.norm(a)
    if th == 0:
        return np.array([0.0, 0, 0, 1])
    return np.concatenate([np.sin(th / 2) * a / th, [np.cos(th / 2)]])


def scene(N1, M, seed=0, noise=0.05):
    """A frame triplet with N1 keypoints in frame i.  Keypoint 0 is a plain
    track; with N1 >= 5: 1 has no partner in frame i-1, 2 none in frame i+1, 3
    an observation in frame i+1 that is 40 px off, 4 a landmark at depth 30;
    with N1 >= 64 also 5 without any partner, 6 with observations that ask for
    a negative inverse depth (the iterate hits the clamp at 1e-4), 7 a partner
    index beyond kps0, and every fourth keypoint from 32 on carries 1 px of
    noise, so that residuals fall on both sides of the gate."""
    rng = np.random.default_rng(seed + 13 * N1 + M)
    poses = np.zeros((3, 7))
    poses[0, :3], poses[0, 3:] = [0.10, 0.004, -0.01], _quat([0.002, -0.01, 0.003])
    poses[1, :3], poses[1, 3:] = [0.01, -0.002, 0.005], _quat([0.001, 0.002, -0.001])
    poses[2, :3], poses[2, 3:] = [-0.09, 0.003, 0.02], _quat([-0.003, 0.012, 0.002])
    intr = np.tile(K_IMAGE, (3, 1))
    depth = rng.uniform(1.0, 2.5, N1)
    if N1 >= 5:
        depth[4] = 30.0
    uv = np.stack([rng.uniform(4, WD - 4, N1), rng.uniform(4, HT - 4, N1)], 1)
    d = 1.0 / depth
    if N1 >= 64:
        d[6] = -0.3
    obs = []
    for o in (0, 2):
        Rij, tij = relative(poses[1], poses[o])
        px, _ = project(Rij, tij, K_IMAGE, uv, d)
        sig = np.full(N1, noise)
        if N1 >= 64:
            sig[32::4] = 1.0
        obs.append(px + rng.standard_normal((N1, 2)) * sig[:, None])
    if N1 >= 5:
        obs[1][3, 0] -= 40.0  # towards a larger inverse depth, so that only the residual gates it
    # the neighbours' keypoint lists: a permutation of the observations plus unmatched rows
    extra = 3
    p0, p2 = rng.permutation(N1 + extra), rng.permutation(N1 + extra)
    kps0 = rng.uniform(0, 60, (N1 + extra, 2))
    kps2 = rng.uniform(0, 60, (N1 + extra, 2))
    kps0[p0[:N1]], kps2[p2[:N1]] = obs[0], obs[1]
    m10, m12 = p0[:N1].astype(np.int64), p2[:N1].astype(np.int64)
    if N1 >= 5:
        m10[1], m12[2] = -1, -1
    if N1 >= 64:
        m10[5] = m12[5] = -1
        m10[7] = N1 + extra  # out of range: no track, nothing read
    disps = rng.uniform(0.3, 1.2, M)
    f = np.float32
    return SimpleNamespace(poses=poses.astype(f), intrinsics=intr.astype(f), disps=disps.astype(f),
                           kps0=kps0.astype(f), kps1=uv.astype(f), kps2=kps2.astype(f), m10=m10,
                           m12=m12, depth=depth, N1=N1, M=M)
