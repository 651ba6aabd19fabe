"""Long-term loop closure on the device, from matched 3-D points to the
corrected map.

Restates dpvo/loop_closure/optim_utils.py:15-17, 64-150, 158-243 and
dpvo/loop_closure/long_term.py:175-203, 235-266 (cuteboyqq/DPVO) on device
tensors:

  `ransac_umeyama`  the Sim3 measurement of a loop from two matched point
                    clouds: 3-point Umeyama hypotheses scored concurrently and
                    the refit on the winner's inliers, two launches
                    (`cuda_ba.ransac_umeyama`, ransac.hip; the reference is
                    numba on the CPU over points copied off the GPU);
  `close_loop`      that measurement joined with the earlier loops and handed
                    to `run_pgo` (the second half of
                    LongTermLoopClosure.close_loop);
  `run_pgo`         the Sim3 pose-graph LM.  The reference evaluates residuals
                    and Jacobians with PyPose Sim3 and
                    torch.autograd.functional.jacobian on the CPU, in a worker
                    process; here one HIP kernel (`cuda_ba.pgo_residual`,
                    pgo.hip) produces residual and both 7x7 Jacobians of every
                    edge, `cuda_ba.solve_system` solves the damped normal
                    equations, and `dpvo_amd.lietorch.Sim3` holds the poses;
  `apply_result`    the optimised poses and scales written back to the map
                    (lc_callback and _rescale_deltas).

Retrieval (DBoW2) and keypoint detection / matching (DISK, LightGlue) are not
part of this module: `close_loop` starts from the frame pair (i, j) and its
two arrays of matched 3-D points, which a caller's own matcher provides.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import global_ba
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


class Sim3Estimate(NamedTuple):
    """Result of `ransac_umeyama`, device tensors: dst ~ s R src + t."""
    R: torch.Tensor            # [3, 3]
    t: torch.Tensor            # [3]
    s: torch.Tensor            # []
    sim3: torch.Tensor         # [8] lietorch data (t, q xyzw with qw >= 0, s)
    num_inliers: torch.Tensor  # [] int32
    mask: torch.Tensor         # [N] bool, inliers of the winning hypothesis
    hypothesis: torch.Tensor   # [] int32, index of the winning sample (-1: none)
    status: torch.Tensor       # [] int32, 0 ok / 1 no inliers / 2 degenerate refit
    info: torch.Tensor         # [4] int32 (num_inliers, hypothesis, stop index, status)


def draw_samples(N, iterations, device, generator=None):
    """[iterations, 3] int32 uniform triples of distinct indices in [0, N):
    the three smallest of N uniform numbers per row."""
    u = torch.rand(iterations, N, device=device, generator=generator)
    return u.argsort(dim=1)[:, :3].to(torch.int32)


def ransac_umeyama(src_points, dst_points, iterations=1, threshold=0.1, samples=None,
                   generator=None, early_exit=100):
    """RANSAC over 3-point Umeyama models and the refit on the winner's inliers
    (optim_utils.py:117-150), dst ~ s R src + t, on the device.

    src_points / dst_points [N, 3] float32 or float64 (the arithmetic is fp64
    either way).  samples [H, 3]: the point triples to try, in the order the
    reference's loop would draw them; with samples=None, `iterations` uniform
    triples of distinct indices are drawn on the device from `generator` (a
    device torch.Generator, or the default one).  The reference draws with an
    unseeded np.random.choice, so what is reproduced is the distribution of
    the samples, not their stream.  Given the samples, the result is the
    reference's: the loop stops after the first hypothesis with more than
    `early_exit` inliers, the best one is the first with the largest count.

    Returns a Sim3Estimate of device tensors (R, t, s and sim3 in the input
    dtype); status 1: no hypothesis had an inlier (the reference returns None,
    here the model is the identity), 2: the refit was degenerate.  No host
    sync when the samples are drawn here; given samples are range-checked,
    which costs one host read (not while a graph is being captured).
    """
    drawn = samples is None
    if drawn:
        samples = draw_samples(src_points.shape[0], iterations, src_points.device, generator)
    model, info, mask = cuda_ba.ransac_umeyama(src_points, dst_points, samples, float(threshold),
                                               int(early_exit), check_samples=not drawn)
    m = model.to(src_points.dtype)
    return Sim3Estimate(m[:9].view(3, 3), m[9:12], m[12], m[13:21], info[0], mask, info[1],
                        info[3], info)


def close_loop(poses_, n, loop_ii, loop_jj, i, j, i_pts, j_pts, min_inliers=30, iterations=400,
               threshold=0.1, samples=None, generator=None, pgo_iters=30):
    """The loop closure of frames (i, j) from their matched 3-D points on
    (long_term.py:235-266): estimate the Sim3 that maps i_pts onto j_pts, join
    it with the relative poses of the earlier loops and optimise the pose graph.

    poses_ [>= n, 7]: the world-to-camera SE3 poses of the map (not modified);
    loop_ii / loop_jj [L] int64 device tensors: the loops closed so far;
    i_pts / j_pts [N, 3] matched points in the two frames.  Returns None when
    there are too few points or inliers, else (final [safe_i, 8] as `run_pgo`
    returns it, loop_ii and loop_jj with (i, j) appended, the Sim3Estimate).
    The first test is `i_pts.numel() < min_inliers`: the reference compares
    numpy's .size, 3 N, with the inlier threshold, and that is kept.  One host
    read (status and inlier count) decides whether the optimiser runs (given
    samples are range-checked before, as in `ransac_umeyama`); the reference's
    worker process and result queue are not reproduced.
    """
    if i_pts.numel() < min_inliers:
        return None
    est = ransac_umeyama(i_pts, j_pts, iterations=iterations, threshold=threshold,
                         samples=samples, generator=generator)
    num_inliers, _, _, status = est.info.tolist()
    if status != 0 or num_inliers < min_inliers:
        return None
    poses_ = poses_.view(-1, 7)
    loop_poses = est.sim3[None].to(poses_.dtype)
    if loop_ii.numel() > 0:  # the first loop has no earlier ones to join
        Gij = SE3(poses_[loop_jj]) * SE3(poses_[loop_ii]).inv()
        loop_poses = torch.cat([SE3_to_Sim3(Gij).data, loop_poses], dim=0)
    new = torch.tensor([i, j], device=loop_ii.device, dtype=loop_ii.dtype)
    loop_ii = torch.cat([loop_ii, new[:1]])
    loop_jj = torch.cat([loop_jj, new[1:]])
    pred_poses = SE3(poses_[:n]).inv()
    final = run_pgo(pred_poses, loop_poses, loop_ii, loop_jj, iters=pgo_iters)
    return final, loop_ii, loop_jj, est


def _delta_sources(pairs, live):
    """Index into `live` (the timestamps of the n keyframes) of the source
    keyframe of every delta record (t1, t0): t0, followed through the records
    while it is itself a removed frame (long_term.py:182-186)."""
    back = {int(t1): int(t0) for t1, t0 in pairs}
    index = {int(t): k for k, t in enumerate(live)}
    out = []
    for t1, _ in pairs:
        t = int(t1)
        for _ in range(len(back) + 1):
            if t not in back:
                break
            t = back[t]
        if t not in index:
            raise ValueError(f"apply_result: delta record {int(t1)} leads to frame {t}, "
                             "which is not a keyframe")
        out.append(index[t])
    return out


def apply_result(final, poses_, patches_, n, M, delta=None, tstamps=None):
    """Write run_pgo's result into the map, in place (lc_callback and
    _rescale_deltas, long_term.py:175-203): poses_[:safe_i] = SE3(res)^-1,
    the inverse depths of the patches of those frames divided by the frame's
    scale, the translation of every delta record scaled by the scale of its
    source keyframe (1 for frames >= safe_i), then PatchGraph.normalize.

    final [safe_i, 8]; poses_ [N, 7]; patches_ [N*M, 3, P, P] (or with a
    leading 1); delta = (log [cap, 7], tstamps [cap, 2] (t1, t0), count) as
    `DevicePatchGraph.keyframe` records it, tstamps [>= n] the keyframes'
    timestamps.  The walk along the records runs on a host copy of the two
    integer tables (one read; loop closures are rare), the scaling is one
    indexed multiply on the device.  Returns normalize's scale.
    """
    inv7, s = split_result(final)
    safe_i = s.shape[0]
    P7 = poses_.view(-1, 7)
    P = patches_.shape[-1]
    K = patches_.view(-1, M, 3, P, P)
    P7[:safe_i] = inv7.to(P7.dtype)
    K[:safe_i, :, 2] /= s.view(safe_i, 1, 1, 1).to(K.dtype)
    log = None
    if delta is not None:
        if tstamps is None:
            raise ValueError("apply_result: the delta log needs tstamps")
        log, pairs, count = delta
        count = int(count)
        if count > 0:
            src = _delta_sources(pairs[:count].tolist(), tstamps[:n].tolist())
            s1 = torch.ones(n, device=log.device, dtype=log.dtype)
            s1[:safe_i] = s.to(log.dtype)
            log[:count, :3] *= s1[torch.tensor(src, device=log.device)][:, None]
    return global_ba.normalize(P7, patches_, n, M, delta=log)
