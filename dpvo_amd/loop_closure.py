"""Loop-closure pose-graph optimisation on the device (P-PGO).

Restates dpvo/loop_closure/optim_utils.py:15-17, 158-243 (cuteboyqq/DPVO) on
device tensors.  The reference evaluates the residuals and their Jacobians
with PyPose Sim3 and torch.autograd.functional.jacobian on the CPU, in a
worker process; here one HIP kernel (`cuda_ba.pgo_residual`, pgo.hip) produces
residual and both 7x7 Jacobians of every edge, `cuda_ba.solve_system` solves
the damped normal equations, and `dpvo_amd.lietorch.Sim3` holds the poses.

Retrieval, keypoint matching and the Umeyama / RANSAC estimate of the loop
measurements are not part of this module: `run_pgo` starts from the loop
edges (`loop_ii`, `loop_jj`) and their measured Sim3 transforms.
"""
from __future__ import annotations

import torch

from .fastba import cuda_ba
from .lietorch import SE3, Sim3


def SE3_to_Sim3(data):
    """SE3 data [..., 7] (or an SE3) -> Sim3 with scale 1 (optim_utils.py:15-17)."""
    if isinstance(data, Sim3):
        return data
    if isinstance(data, SE3):
        data = data.data
    return Sim3(torch.cat([data, torch.ones_like(data[..., :1])], dim=-1))


def _sim3_data(x):
    return x.data if isinstance(x, Sim3) else x


def _chain_constants(input_poses):
    """dSij = T_{k-1} T_k^-1, k = 1 .. n-1, with T = Sim3(input_poses)^-1
    (optim_utils.py:168-178): the measured odometry steps."""
    T = SE3_to_Sim3(input_poses).inv()
    return (T[:-1] * T[1:].inv()).data


def _edges(n, dSij, dSloop, ii, jj):
    """Constants and indices of the whole graph: the odometry chain (k, k-1)
    followed by the loop edges (optim_utils.py:171-182)."""
    kk = torch.arange(1, n, device=dSij.device)
    constants = torch.cat([dSij, _sim3_data(dSloop).to(dSij.dtype)], dim=0).contiguous()
    return constants, torch.cat([kk, ii]), torch.cat([kk - 1, jj])


def residual(Ginv, input_poses, dSloop, ii, jj, jacobian=False):
    """Residuals [r, 7] of the odometry chain and the loop edges at the pose
    tangents Ginv [n, 7]; with jacobian=True also (J_Ginv_i, J_Ginv_j, iii, jjj),
    the inputs of cuda_ba.solve_system (optim_utils.py:163-189)."""
    constants, iii, jjj = _edges(Ginv.shape[0], _chain_constants(input_poses).to(Ginv.dtype),
                                 dSloop, ii, jj)
    return _residual(Ginv, constants, iii, jjj, jacobian)


def _residual(Ginv, constants, iii, jjj, jacobian):
    out = cuda_ba.pgo_residual(Ginv.contiguous(), constants, iii, jjj, jacobian)
    if not jacobian:
        return out[0]
    return out[0], (out[1], out[2], iii, jjj)


def _mean_square(r):
    return r.double().square().mean().item()


def _lm_iteration(Ginv, constants, iii, jjj, ep, lmbda, freen):
    """One iteration of optim_utils.py:226-238: (Ginv, lmbda, mean square before the step)."""
    resid, (J_i, J_j, _, _) = _residual(Ginv, constants, iii, jjj, True)
    before = _mean_square(resid)
    delta, = cuda_ba.solve_system(J_i, J_j, iii, jjj, resid, ep, lmbda, freen)
    Ginv_tmp = Ginv + delta.to(Ginv.dtype)
    if _mean_square(_residual(Ginv_tmp, constants, iii, jjj, False)) < before:
        return Ginv_tmp, lmbda / 2, before
    return Ginv, lmbda * 2, before


def perform_updates(input_poses, dSloop, ii_loop, jj_loop, iters, ep=0.0, lmbda=1e-6,
                    fix_opt_window=False):
    """Levenberg-Marquardt over the Sim3 pose graph (optim_utils.py:211-243).

    input_poses: SE3 data [n, 7]; dSloop: Sim3 (or its data [L, 8]) of the loop
    measurements; ii_loop / jj_loop [L] int64.  The variables are the tangents
    Ginv = Log(Sim3(input_poses)^-1); returns the optimised poses Exp(Ginv)^-1,
    a Sim3 in the frame of input_poses.  The control flow is the
    reference's: a step is kept when it lowers the mean square residual (formed
    in fp64), lmbda is halved or doubled, and the loop ends early once the
    residual is below 1e-5 and improved by less than 1.5x over four iterations.
    """
    if isinstance(input_poses, SE3):
        input_poses = input_poses.data
    input_poses = input_poses.clone()
    freen = torch.cat((ii_loop, jj_loop)).max().item() + 1 if fix_opt_window else -1

    Ginv = SE3_to_Sim3(input_poses).inv().log()
    # the graph is the same in every iteration: build its constants once
    constants, iii, jjj = _edges(Ginv.shape[0], _chain_constants(input_poses), dSloop,
                                 ii_loop, jj_loop)
    history = []
    for itr in range(iters):
        Ginv, lmbda, ms = _lm_iteration(Ginv, constants, iii, jjj, ep, lmbda, freen)
        history.append(ms)
        if history[-1] < 1e-5 and itr >= 4 and history[-5] / history[-1] < 1.5:
            break
    return Sim3.exp(Ginv).inv()


def run_pgo(pred_poses, loop_poses, loop_ii, loop_jj, iters=30):
    """Optimise and re-anchor (optim_utils.py:202-209): the result is moved so
    that pose safe_i = loop_ii.max() + 1, the first pose after the loop, keeps
    its input value, and cut to [:safe_i].  Returns Sim3 data [safe_i, 8]."""
    if isinstance(pred_poses, SE3):
        pred_poses = pred_poses.data
    n = pred_poses.shape[0]
    safe_i = int(loop_ii.max().item()) + 1
    if safe_i >= n:
        raise ValueError(f"run_pgo: loop_ii.max() = {safe_i - 1} must be below n - 1 = {n - 1} "
                         "(the pose after the loop anchors the result)")
    final = perform_updates(pred_poses, loop_poses, loop_ii, loop_jj, iters=iters)
    anchor = SE3_to_Sim3(pred_poses)
    final = (anchor[safe_i:safe_i + 1] * final[safe_i:safe_i + 1].inv()) * final
    return final.data[:safe_i]


def split_result(final):
    """run_pgo's [safe_i, 8] -> (SE3 data of the inverse [safe_i, 7], scale
    [safe_i]): the poses to store and the factor to divide patch depths by
    (long_term.py:196-200)."""
    res, s = _sim3_data(final).split([7, 1], dim=-1)
    return SE3(res).inv().data, s.squeeze(-1)
