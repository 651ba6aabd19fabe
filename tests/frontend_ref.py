"""fp64 restatement of the frame front-end and the trajectory read-out
(dpvo_amd/frontend.py, csrc/frontend.hip), on the CPU, built on
tests/se3_restatement.py (from_data, Log, Exp, mul, inv, to_data: 4x4
matrices, matrix exponential, no closed-form coefficient -- nothing shared
with the kernels).

  motion_model   dpvo/dpvo.py:943-957
  lower_median   what torch.median returns (dpvo.py:962)
  init_frame     dpvo.py:931-965 on NumPy copies of the per-frame buffers
  get_pose / trajectory   dpvo.py:385-417, the recursion over a dict written
                 as the reference writes it
"""
import numpy as np
import torch

import se3_restatement as R


def _mat(d):
    return R.from_data(torch.as_tensor(np.asarray(d, np.float64)))


def _data(M):
    return R.to_data(M).numpy()


def time_factor(times, counter):
    """*_, a, b, c = [1] * 3 + tlist; fac = (c - b) / (b - a) (dpvo.py:949-950),
    tlist = times[:counter + 1].  b == a: 1 (the reference raises)."""
    tl = [1.0] * 3 + [float(t) for t in np.asarray(times)[:counter + 1]]
    a, b, c = tl[-3:]
    return 1.0 if b == a else (c - b) / (b - a)


def motion_model(P1, P2, fac, damping):
    """Exp(damping * fac * Log(P1 * P2^-1)) * P1 as SE3 data [7] (fp64)."""
    A, B = _mat(P1), _mat(P2)
    xi = (damping * fac) * R.Log(R.mul(A, R.inv(B)))
    return _data(R.mul(R.Exp(xi), A))


def lower_median(x):
    x = np.asarray(x).reshape(-1)
    if np.isnan(x).any():
        return x.dtype.type(np.nan)
    return np.sort(x)[(len(x) - 1) // 2]


def init_frame(poses, patches, intrinsics, tstamps, times, new_patches, new_intrinsics, n, counter,
               M, motion_model_name="DAMPED_LINEAR", damping=0.5, res=4.0, median=True):
    """Returns (poses, patches, intrinsics, tstamps) after dpvo.py:931-965; the
    pose row in fp64 (the caller compares after rounding), the rest in the
    buffers' own dtypes."""
    poses = np.asarray(poses).astype(np.float64)
    patches = np.array(patches, copy=True)
    intrinsics = np.array(intrinsics, copy=True)
    tstamps = np.array(tstamps, copy=True)
    P = patches.shape[-1]
    tstamps[n] = counter
    intrinsics[n] = (torch.as_tensor(np.asarray(new_intrinsics, np.float32)) / res).numpy()
    if n > 1:
        if motion_model_name == "DAMPED_LINEAR":
            poses[n] = motion_model(poses[n - 1], poses[n - 2], time_factor(times, counter),
                                    damping)
        else:
            poses[n] = poses[n - 1]
    new = np.array(new_patches, copy=True).reshape(M, 3, P, P)
    if median and n >= 1:
        new[:, 2] = lower_median(patches[max(n - 3, 0) * M:n * M, 2])
    patches[n * M:(n + 1) * M] = new
    return poses, patches, intrinsics, tstamps


def get_pose(traj, delta, t):
    """dpvo.py:385-390 on 4x4 matrices."""
    if t in traj:
        return traj[t]
    t0, dP = delta[t]
    return R.mul(dP, get_pose(traj, delta, t0))


def trajectory(poses, tstamps, n, records, counter, inverse=True):
    """terminate's interpolation (dpvo.py:404-411).  records: (t1, t0, dP [7]) in
    log order, entered into a dict (the last record of a t1 wins); records with
    t0 >= t1 or an index outside [0, counter) are ignored (the reference would
    recurse forever or raise) and counted.  A frame whose recursion finds no
    entry is unresolved: NaN row, root -1.
    Returns (traj [counter, 7] fp64, root [counter], info [2])."""
    traj, rootof = {}, {}
    for i in range(n):
        traj[int(tstamps[i])] = _mat(poses[i])
        rootof[int(tstamps[i])] = i
    delta, ignored = {}, 0
    for t1, t0, dP in records:
        t1, t0 = int(t1), int(t0)
        if t0 >= t1 or t0 < 0 or t1 >= counter:
            ignored += 1
            continue
        delta[t1] = (t0, _mat(dP))
    out = np.full((counter, 7), np.nan)
    root = np.full(counter, -1, np.int64)
    unresolved = 0
    for t in range(counter):
        try:
            G = get_pose(traj, delta, t)
        except KeyError:
            unresolved += 1
            continue
        out[t] = _data(R.inv(G) if inverse else G)
        r = t
        while r not in traj:
            r = delta[r][0]
        root[t] = rootof[r]
    return out, root, np.array([unresolved, ignored], np.int32)
