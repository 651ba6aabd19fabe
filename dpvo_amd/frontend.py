"""Frame front-end and trajectory read-out on the device (csrc/frontend.hip).

init_frame   the head of DPVO.__call__ (dpvo/dpvo.py:931-965): timestamp index,
             intrinsics / RES, the motion-model pose and the median-depth
             patches of the new frame, one launch of one workgroup.
trajectory   DPVO.terminate's interpolation (dpvo.py:385-417): get_pose(t) for
             every frame from the keyframe poses and the pg.delta log that
             DevicePatchGraph.keyframe records.
append_delta the pg.delta record of a frame dropped before initialisation
             (dpvo.py:977).

Nothing here synchronises with the host; with device-scalar n / counter
init_frame replays from a captured graph.
"""
from __future__ import annotations

import torch

from ._native import load_extension, require_gpu


def _scalar(v, name):
    """(host int, int32 device tensor or None) of an int-or-tensor argument."""
    if isinstance(v, torch.Tensor):
        require_gpu(v)
        if v.dtype != torch.int32:
            raise TypeError(f"{name} as a tensor must be an int32 device scalar")
        return 0, v
    return int(v), None


def init_frame(poses, patches, intrinsics, tstamps, times, new_patches, new_intrinsics, n, counter,
               M, *, motion_model="DAMPED_LINEAR", damping=0.5, res=4.0, median=True):
    """Seed frame row n of the per-frame buffers, in place (dpvo.py:931-965).

    poses [N,7], patches [N*M,3,P,P], intrinsics [N,4] (float32), tstamps [N]
    (int64) are the per-frame buffers; times [cap] (float64, device) holds the
    caller's frame times by frame counter, times[counter] written before the
    call.  new_patches is the patchifier's [M,3,P,P] or [1,M,3,P,P],
    new_intrinsics [4].  n / counter: a Python int, or an int32 device scalar
    (graph replay).

      tstamps[n] = counter; intrinsics[n] = new_intrinsics / res
      n > 1: poses[n] = Exp(damping * fac * Log(P1 * P2^-1)) * P1 with
             fac = (c - b) / (b - a) over the last three times
             (motion_model "DAMPED_LINEAR"; fac = 1 where b == a, the reference
             raises ZeroDivisionError), or poses[n-1] (any other string, the
             reference's else)
      patches rows of frame n = new_patches, their depth channel replaced by
             the lower median of the depths of frames [max(n-3, 0), n) when
             median and n >= 1 (torch.median's value; NaN if any is NaN)

    The reference's torch.rand_like depth before initialisation stays the
    caller's: pass median=False (or n = 0) and put it in new_patches."""
    ext = load_extension("cuda_ba")
    require_gpu(poses)
    n_host, n_dev = _scalar(n, "n")
    c_host, c_dev = _scalar(counter, "counter")
    P = patches.shape[-1]
    ext.frame_init(poses, patches, intrinsics, tstamps, times, new_patches.reshape(-1, 3, P, P),
                   new_intrinsics.reshape(-1), int(M), n_host, n_dev, c_host, c_dev,
                   1 if motion_model == "DAMPED_LINEAR" else 0, float(damping), float(res),
                   bool(median))


def trajectory(poses, tstamps, n, delta, counter, inverse=True):
    """get_pose(t) for t in [0, counter) (dpvo.py:385-417) -> (traj, root, info).

    poses [N,7] / tstamps [N]: the keyframe buffers, n keyframes (Python int or
    int32 device scalar).  delta = (log [cap,7], pairs [cap,2] (t1, t0), count
    int32[1]) as DevicePatchGraph.keyframe(delta=...) fills it.  counter: the
    number of frames (Python int; it sizes the launches).

    traj [counter,7] float32: the pose of every frame, inverted when `inverse`
    (terminate returns poses.inv()); root [counter] int64: the row of `poses`
    the frame hangs on (-1: unresolved, its traj row is NaN); info int32[2] =
    {unresolved frames, ignored records}.  A keyframe wins over a record for
    the same frame; of several records for one frame the last in log order
    wins; records with t0 >= t1 or an index outside [0, counter) are ignored."""
    ext = load_extension("cuda_ba")
    require_gpu(poses)
    log, pairs, count = delta
    n_host, n_dev = _scalar(n, "n")
    traj, root, info = ext.trajectory(poses, tstamps, n_host, n_dev, log, pairs, count,
                                      int(counter), bool(inverse))
    return traj, root, info


def append_delta(delta, t1, t0, dP=None):
    """pg.delta[t1] = (t0, dP) appended to delta = (log, pairs, count) with
    device-side torch ops and no host sync (dpvo.py:977 with dP=None: the
    identity).  t1 / t0: Python ints or device integer tensors.  When the log
    is full nothing is written and the count stays (the analogue of the patch
    graph's error bit 8 of keyframe()); the returned bool device tensor [1]
    tells whether the record was kept."""
    log, pairs, count = delta
    require_gpu(log)
    cap = log.shape[0]
    dev = log.device
    if dP is None:
        row = torch.zeros(7, dtype=log.dtype, device=dev)
        row[6] = 1.0
    else:
        row = dP.to(device=dev, dtype=log.dtype).reshape(7)
    if isinstance(t1, torch.Tensor) or isinstance(t0, torch.Tensor):
        pr = torch.stack([torch.as_tensor(t1, device=dev).reshape(()).to(pairs.dtype),
                          torch.as_tensor(t0, device=dev).reshape(()).to(pairs.dtype)])
    else:
        pr = torch.tensor([int(t1), int(t0)], dtype=pairs.dtype, device=dev)
    slot = count.reshape(1).to(torch.long)
    ok = slot < cap
    if cap == 0:
        return ok
    idx = slot.clamp(0, cap - 1)
    log.index_copy_(0, idx, torch.where(ok[:, None], row[None], log[idx]))
    pairs.index_copy_(0, idx, torch.where(ok[:, None], pr[None], pairs[idx]))
    count.add_(ok.to(count.dtype).reshape(count.shape))
    return ok
