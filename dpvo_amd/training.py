"""The loss and the optimiser step of DPVO's train.py (85-139) on the MI355X.

``flow_loss`` and ``pose_loss`` are autograd Functions over the fused HIP
kernels of csrc/train.hip (one launch each way, fp64 inside, fixed-order sums:
two calls give identical bits; no host synchronisation).  ``sequence_loss``
restates the loop of train.py:85-118 over a trajectory of ``VONet.forward``
and ``train_step`` the step of train.py:77-125.  The data readers that feed it
are dpvo_amd.data_readers (scripts/train.py is the loop); the logger and
checkpoint rotation are not part of this module.
"""
from __future__ import annotations

import torch

from .fastba import cuda_ba
from .lietorch import SE3


class _FlowLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, coords_gt, valid):
        loss, count, emin, argmin = cuda_ba.flow_loss_forward(coords, coords_gt, valid)
        ctx.save_for_backward(coords, coords_gt, valid, count, argmin)
        n = count[0]
        ctx.mark_non_differentiable(n, emin)
        return loss[0], n, emin

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gc, _ge):
        coords, coords_gt, valid, count, argmin = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        gx = cuda_ba.flow_loss_backward(coords, coords_gt, valid, count, argmin,
                                        g.to(torch.float32).reshape(1))
        return gx.view(coords.shape), None, None


def flow_loss(coords, coords_gt, valid):
    """train.py:87-88: per edge the minimum over the P x P points of
    |coords - coords_gt|, averaged over the edges whose centre is valid.

    coords, coords_gt [.., E, P, P, 2] (P 1 or 3), valid [.., E] (the patch
    centre's, as ``transform(.., jacobian=True)`` returns it) or [.., E, P, P]
    (the centre is taken) -> (loss, count, emin): the mean (0-d), the number
    of valid edges (0-d int32) and the per-edge minima [E] (of every edge; the
    ``px1`` metric masks them).  Only ``coords`` is differentiable: the
    gradient is g (x - y) / |x - y| / count at each valid edge's argmin (ties:
    the lowest point index; an exactly-zero difference: zero).

    Deviation from the reference: with no valid edge the loss is 0 with a zero
    gradient; the reference returns the mean of an empty tensor, NaN."""
    P = coords.shape[-2]
    E = coords.numel() // (2 * P * P)
    if valid.numel() == E * P * P and P > 1:
        valid = valid.reshape(E, P, P)[:, P // 2, P // 2]
    return _FlowLoss.apply(coords, coords_gt, valid.reshape(E).to(torch.float32))


class _PoseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, Ps):
        out, tr, ro = cuda_ba.pose_loss_forward(G, Ps)
        ctx.save_for_backward(G, Ps)
        s = out[2]
        ctx.mark_non_differentiable(tr, ro, s)
        return out[0], out[1], tr, ro, s

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_tr, g_ro, _a, _b, _c):
        G, Ps = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        z = G.new_zeros(())
        g = torch.stack([z if g_tr is None else g_tr.to(torch.float32),
                         z if g_ro is None else g_ro.to(torch.float32)])
        gG = cuda_ba.pose_loss_backward(G, Ps, g)
        return torch.nn.functional.pad(gG, (0, 1)).view(G.shape), None


def pose_loss(Gs, Ps):
    """train.py:90-113 for n <= 32 poses: Gs, Ps SE3 (or pose data) [1, n, 7]
    -> (tr, ro, tr_pairs, ro_pairs, s).  A_i = inv(G_i) with its translation
    scaled by s = kabsch_umeyama(t_gt, t_est).clamp(max=10) (a constant in the
    backward), B_i = inv(Ps_i), e_ij = Log((A_i^-1 A_j)(B_i^-1 B_j)^-1) over all
    ordered pairs i != j; tr / ro are the means of |e[:3]| / |e[3:]|, the pairs
    come in ``meshgrid(.., 'ij')`` order with the diagonal removed.  Only Gs is
    differentiable (a left-tangent row padded to the embedding size).  n < 2:
    zeros."""
    G = Gs.data if isinstance(Gs, SE3) else Gs
    P = Ps.data if isinstance(Ps, SE3) else Ps
    return _PoseLoss.apply(G, P.detach())


def sequence_loss(traj, P=3, flow_weight=0.1, pose_weight=10.0, structure_only=False):
    """The loss of train.py:85-120 over a trajectory of ``VONet.forward`` ->
    (loss, metrics).  The pose term is added for steps i >= 2 and only when not
    structure-only.  ``metrics`` (of the last step, as train.py:129-139) are
    0-d device tensors: nothing here synchronises with the host."""
    if len(traj) == 0:
        raise ValueError("sequence_loss: the trajectory is empty (STEPS = 0)")
    loss = 0.0
    for i, (v, x, y, P1, P2, kl) in enumerate(traj):
        if x.shape[-2] != P:
            raise ValueError(f"sequence_loss: coords have P = {x.shape[-2]}, expected {P}")
        e, count, emin = flow_loss(x, y, v)
        tr, ro, trp, rop, _ = pose_loss(P1, P2)
        loss = loss + flow_weight * e
        if not structure_only and i >= 2:
            loss = loss + pose_weight * (tr + ro)
    loss = loss + kl  # 0 (no longer used), a device tensor here
    ok = (v.reshape(-1) > 0.5).to(torch.float32)
    metrics = {
        "loss": loss.detach(),
        "kl": kl,
        "px1": ((emin < 0.25).to(torch.float32) * ok).sum() / count.clamp(min=1),
        "ro": ro.detach(),
        "tr": tr.detach(),
        "r1": (rop < 0.001).float().mean(),
        "r2": (rop < 0.01).float().mean(),
        "t1": (trp < 0.001).float().mean(),
        "t2": (trp < 0.01).float().mean(),
    }
    return loss, metrics


def train_step(net, optimizer, images, poses, disps, intrinsics, *, steps=18, clip=10.0,
               scheduler=None, structure_only=False, **forward_kw):
    """One optimiser step (train.py:77-125): zero_grad, ``net(...)`` with
    STEPS = ``steps``, ``sequence_loss``, backward, ``clip_grad_norm_``, step
    (and ``scheduler.step()``).  ``poses`` are the ground-truth SE3 as the
    loader's ``SE3(poses).inv()``.  Returns (loss, metrics), device tensors."""
    optimizer.zero_grad()
    traj = net(images, poses, disps, intrinsics, STEPS=steps, structure_only=structure_only,
               **forward_kw)
    loss, metrics = sequence_loss(traj, P=net.P, structure_only=structure_only)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return loss.detach(), metrics


__all__ = ["flow_loss", "pose_loss", "sequence_loss", "train_step"]
