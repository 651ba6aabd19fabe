"""Trajectory evaluation on the device (csrc/evaluate.hip): poses in, score out.

ate        the absolute trajectory error of evaluate_euroc.py:109-119, which the
           reference takes from evo: association by timestamp
           (sync.associate_trajectories), Sim(3) Umeyama alignment
           (align=True, correct_scale=True) and the statistics of the
           translation error, in one launch and without a host read.
read_tum / write_tum   the TUM text format `t x y z qx qy qz qw` (host, numpy).

The association rule is written out in include/dpvo_hot.h; it is evo's as
restated there, not checked against evo itself.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from ._native import load_extension, require_gpu


class ATEResult(NamedTuple):
    """Device tensors; reading any of them is the caller's synchronisation."""
    stats: torch.Tensor   # float64 [8] = rmse, mean, median, std, min, max, sse, count
    model: torch.Tensor   # float64 [13] = R (row-major), t, c:  ref ~ c R est + t
    pairs: torch.Tensor   # int32 [min(n, m), 2] = (est index, ref index), unused rows -1
    status: torch.Tensor  # int32 [1]: bit 0 < 3 pairs, bit 1 degenerate, bit 2 unsorted stamps

    @property
    def rmse(self):
        return self.stats[0]


def _f64(x, like):
    return torch.as_tensor(x, dtype=torch.float64, device=like.device)


def ate(traj, tstamps, ref_xyz, ref_t, max_diff=0.01, align=True):
    """ATE of traj against a reference trajectory -> ATEResult.

    traj [n, >= 3] (float32 or float64, device): DPVO.terminate's poses; the
    first three columns are used.  tstamps [n], ref_xyz [m, >= 3], ref_t [m]:
    anything torch.as_tensor takes, moved to traj's device as float64.  Both
    stamp arrays must be non-decreasing (status bit 2 otherwise).  n, m <=
    65536.  On a set status bit stats[0:7] are NaN and stats[7] is the pair
    count."""
    ext = load_extension("cuda_ba")
    require_gpu(traj)
    if traj.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"ate: traj must be float32 or float64, got {traj.dtype}")
    est_xyz = traj[:, :3]
    ref_xyz = _f64(ref_xyz, traj)[:, :3]
    stats, model, pairs, status = ext.trajectory_ate(est_xyz, _f64(tstamps, traj), ref_xyz,
                                                     _f64(ref_t, traj), float(max_diff),
                                                     bool(align))
    return ATEResult(stats, model, pairs, status)


def read_tum(path):
    """`t x y z qx qy qz qw` per line (# comments; spaces or commas, as EuRoC's
    converted ground truth has them) -> (tstamps float64 [n], poses float64 [n, 7])."""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].replace(",", " ").split()
            if not line:
                continue
            if len(line) < 8:
                raise ValueError(f"{path}: expected 8 numbers per line, got {len(line)}")
            rows.append([float(v) for v in line[:8]])
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    return a[:, 0].copy(), a[:, 1:].copy()


def write_tum(path, poses, tstamps):
    """poses [n, 7] (t, then the quaternion x y z w) and tstamps [n] -> TUM text."""
    poses = np.asarray(torch.as_tensor(poses).detach().cpu(), dtype=np.float64).reshape(-1, 7)
    tstamps = np.asarray(torch.as_tensor(tstamps).detach().cpu(), dtype=np.float64).reshape(-1)
    if len(poses) != len(tstamps):
        raise ValueError(f"write_tum: {len(poses)} poses, {len(tstamps)} stamps")
    with open(path, "w") as f:
        for t, p in zip(tstamps, poses):
            f.write(" ".join([repr(float(t))] + [repr(float(v)) for v in p]) + "\n")
