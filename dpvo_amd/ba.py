"""The training path of dpvo/ba.py: the differentiable
Gauss-Newton layer BA (88-297) as fused HIP forward and backward kernels
(ba_layer.hip), python_ba_wrapper (299-415) on its forward, and the dense
block solves the reference builds the layer from.

The reference (dpvo/ba.py:13-38, 59-77) solves its damped pose system with
torch.linalg.cholesky_ex + cholesky_solve inside an autograd Function that
returns zeros (and no gradient) when the factorisation fails.  Here the
factor and both triangular sweeps are this build's batched HIP kernel
(spd_solve.hip, through cuda_ba.spd_solve / spd_solve_factored and the C ABI
dpvo_spd_solve); the gradient reuses the stored factor.

Gradient of x = H^-1 b (H symmetric):  db = H^-1 g,  dH = -x db^T  (the same
expression the reference returns: it treats H as unconstrained, so the caller
symmetrises if it needs to).  The per-frame inference BA does not come here
(it runs the fused fastba kernels).
"""
from __future__ import annotations

import torch

from ._native import load_extension

_cuda_ba = load_extension("cuda_ba")


def _require_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU (HIP) tensor; the MI355X build has no CPU path")


class CholeskySolver(torch.autograd.Function):
    """x = H^-1 b for SPD H [..., n, n], b [..., n, k] (replaces dpvo/ba.py:13-38).
    A failed factorisation anywhere in the batch gives x = 0 and no gradient,
    the reference's "don't crash training" rule."""

    @staticmethod
    def forward(ctx, H, b):
        _require_gpu(H, "H")
        _require_gpu(b, "b")
        x, L, info = _cuda_ba.spd_solve(H, b)
        ctx.failed = bool(torch.any(info))  # one host sync, as the reference's torch.any
        if ctx.failed:
            return torch.zeros_like(b)
        ctx.save_for_backward(L, x)
        return x

    @staticmethod
    def backward(ctx, grad_x):
        if ctx.failed:
            return None, None
        L, x = ctx.saved_tensors
        db = _cuda_ba.spd_solve_factored(L, grad_x.contiguous())
        dH = -(x @ db.transpose(-1, -2))
        return dH, db


def _blocks_to_dense(A):
    """[b, n, m, p, q] block matrix -> dense [b, n p, m q]."""
    b, n, m, p, q = A.shape
    return A.transpose(2, 3).reshape(b, n * p, m * q)


def _dense_to_blocks(X, n, p, m, q):
    """dense [b, n p, m q] -> [b, n, m, p, q] block matrix."""
    return X.reshape(X.shape[0], n, p, m, q).transpose(2, 3)


def block_matmul(A, B):
    """Block matrix product C_ij = sum_k A_ik B_kj (dpvo/ba.py:59-65):
    A [b, n1, m1, p1, q1], B [b, m1, m2, q1, q2] -> [b, n1, m2, p1, q2]."""
    _, n1, _, p1, _ = A.shape
    _, _, m2, _, q2 = B.shape
    return _dense_to_blocks(_blocks_to_dense(A) @ _blocks_to_dense(B), n1, p1, m2, q2)


def block_solve(A, B, ep=1.0, lm=1e-4):
    """Damped block solve (dpvo/ba.py:67-77): X = (A + diag(ep + lm diag A))^-1 B
    on the dense form, A [b, n, n, p, p], B [b, n, m, p, q] -> [b, n, m, p, q]."""
    _, n1, _, p1, _ = A.shape
    _, _, m2, _, q2 = B.shape
    Ad = _blocks_to_dense(A)
    Ad = Ad + torch.diag_embed(ep + lm * torch.diagonal(Ad, dim1=-2, dim2=-1))
    X = CholeskySolver.apply(Ad, _blocks_to_dense(B))
    return _dense_to_blocks(X, n1, p1, m2, q2)


class _BALayer(torch.autograd.Function):
    """(pose data [1, N, 7], patches [1, M, 3, p, p], targets, weights) ->
    (dX [n_free, 6], dZ [M]) of one Gauss-Newton step: the fused forward and
    backward of ba_layer.hip.  The pose gradient is a left-tangent row padded
    to the embedding size, lietorch's convention.  The failed-factorisation
    flag stays in the workspace and predicates the backward on the device."""

    @staticmethod
    def forward(ctx, pdata, patches, targets, weights, intrinsics, lmbda, ii, jj, kk, bounds, ep,
                n, fixedp, structure_only):
        for t, name in ((pdata, "poses"), (patches, "patches"), (targets, "targets"),
                        (weights, "weights"), (intrinsics, "intrinsics")):
            _require_gpu(t, name)
        need_grad = any(ctx.needs_input_grad[:4])
        pdata, patches, intrinsics = pdata.contiguous(), patches.contiguous(), intrinsics.contiguous()
        lm_t, lm_f = (lmbda, 0.0) if isinstance(lmbda, torch.Tensor) else (None, float(lmbda))
        dX, dZ, ws = _cuda_ba.ba_layer_forward(pdata, patches, intrinsics, targets, weights, lm_t,
                                               lm_f, ii, jj, kk, n, fixedp, structure_only,
                                               list(bounds), float(ep), need_grad)
        ctx.args = (n, fixedp, structure_only)
        ctx.save_for_backward(ws, pdata, patches, intrinsics, ii, jj, kk)
        ctx.mark_non_differentiable(ws)
        return dX, dZ, ws

    @staticmethod
    def backward(ctx, gX, gZ, _gws):
        ws, pdata, patches, intrinsics, ii, jj, kk = ctx.saved_tensors
        n, fixedp, structure_only = ctx.args
        if gX is None:
            gX = pdata.new_zeros((0 if structure_only else n - fixedp, 6))
        if gZ is None:
            gZ = pdata.new_zeros(patches.shape[-4])
        gT, gW, gP, gK = _cuda_ba.ba_layer_backward(ws, pdata, patches, intrinsics, ii, jj, kk,
                                                    gX.contiguous(), gZ.contiguous(), n, fixedp,
                                                    structure_only)
        gpose = torch.nn.functional.pad(gP, (0, 1)).view(pdata.shape)
        c = patches.shape[-1] // 2
        gpatch = torch.zeros_like(patches)
        gpatch[..., c, c] = gK.view(patches.shape[:-2])
        E = ii.numel()
        return (gpose, gpatch, gT.view(1, E, 2), gW.view(1, E, 2)) + (None,) * 10


def layer_status(ws):
    """The two status words of a BA call's workspace as an int32 device tensor:
    [edges closed for an out-of-range index, factorisation info (0 = ok)]."""
    return ws[:8].view(torch.int32)


def BA(poses, patches, intrinsics, targets, weights, lmbda, ii, jj, kk, bounds, ep=100.0,
       PRINT=False, fixedp=1, structure_only=False, num_poses=None, return_status=False):
    """One differentiable Gauss-Newton step: dpvo/ba.py BA (88-297), B = 1.

    poses SE3 [1, N, 7], patches [1, M, 3, p, p], intrinsics [1, N, 4], targets
    and weights [1, E, 2], ii / jj / kk int64 [E] -> (SE3, patches).  Gradients
    reach poses, patches, targets and weights.  Deviations from the reference:
    all reductions are fp64 in a fixed order (two calls are bit-identical);
    ``intrinsics`` and ``lmbda`` (a float or a 1-element tensor, > 0) get no
    gradient; an edge with an index outside [0, n) / [0, M) is closed and
    counted instead of read.  With ``num_poses`` given (n, the reference's
    max(ii, jj) + 1) neither direction synchronises with the host; None
    computes it as the reference does, at the cost of one sync.  ``bounds`` is
    a sequence of 4 floats (a device tensor is read back, one sync)."""
    from .lietorch import SE3

    pdata = poses.data if isinstance(poses, SE3) else poses
    if pdata.dim() != 3 or pdata.shape[0] != 1 or patches.shape[0] != 1:
        raise ValueError("BA: batch size 1 (poses [1, N, 7], patches [1, M, 3, p, p])")
    if num_poses is None:
        n = int(torch.maximum(ii.max(), jj.max())) + 1 if ii.numel() else fixedp
    else:
        n = int(num_poses)
    if isinstance(bounds, torch.Tensor):
        bounds = bounds.tolist()
    if isinstance(lmbda, torch.Tensor):
        if lmbda.numel() != 1:
            raise ValueError("BA: lmbda must be a float or a 1-element tensor")
        lmbda = lmbda.detach()
    elif not lmbda > 0:
        raise ValueError("BA: lmbda > 0 is required")
    N = pdata.shape[1]
    n = min(max(n, fixedp), N)
    dX, dZ, ws = _BALayer.apply(pdata, patches, targets, weights, intrinsics, lmbda, ii, jj, kk,
                                tuple(float(b) for b in bounds), ep, n, fixedp, bool(structure_only))
    if PRINT:  # the reference's mean gated residual (ba.py:173-174); synchronises
        print(_mean_gated_residual(pdata, patches, intrinsics, targets, ii, jj, kk, bounds))
    x, y, disps = patches.unbind(dim=2)
    disps = (disps + dZ.view(1, -1, 1, 1)).clamp(min=1e-3, max=10.0)
    out_patches = torch.stack([x, y, disps], dim=2)
    out = SE3(pdata)
    if not structure_only and n - fixedp > 0:
        out = out.retr(torch.nn.functional.pad(dX, (0, 0, fixedp, N - n)).view(1, N, 6))
        # a failed factorisation leaves the poses as they were, bit for bit (the
        # lietorch ops renormalise quaternions even for a zero step); the flag
        # is read on the device
        out = SE3(torch.where(layer_status(ws)[1] != 0, pdata, out.data))
    if return_status:
        return out, out_patches, layer_status(ws)
    return out, out_patches


def _mean_gated_residual(pdata, patches, intrinsics, targets, ii, jj, kk, bounds):
    from . import projective_ops as pops
    from .lietorch import SE3

    with torch.no_grad():
        coords, v = pops.transform(SE3(pdata), patches, intrinsics, ii, jj, kk, valid=True)
        p = coords.shape[3]
        c = coords[..., p // 2, p // 2, :]
        r = targets - c
        v = v[..., p // 2, p // 2] * (r.norm(dim=-1) < 250).to(r.dtype)
        v = v * ((c[..., 0] > bounds[0]) & (c[..., 1] > bounds[1]) & (c[..., 0] < bounds[2]) &
                 (c[..., 1] < bounds[3])).to(r.dtype)
        return (r * v[..., None]).norm(dim=-1).mean().item()


def python_ba_wrapper(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, PPF, t0, t1,
                      iterations, eff_impl=False):
    """dpvo/ba.py python_ba_wrapper (299-415), the fork's per-frame BA call:
    ``iterations`` BA steps with bounds [0, 0, W-1, H-1] (W = int(2 max cx),
    H = int(2 max cy)), fixedp = t0, structure_only = (t1 == t0), ep = 100,
    under no_grad.  ``patches`` is updated in place, as is a ``poses`` tensor;
    returns the pose tensor.  PPF and eff_impl are accepted and ignored."""
    from .lietorch import SE3

    is_group = isinstance(poses, SE3)
    pdata = poses.data if is_group else poses
    with torch.no_grad():
        shape = pdata.shape
        cur = SE3(pdata.reshape(1, -1, 7))
        K = intrinsics.reshape(1, -1, 4)
        H = int(2 * K[..., 3].max().item())
        W = int(2 * K[..., 2].max().item())
        bounds = (0.0, 0.0, W - 1.0, H - 1.0)
        n = int(torch.maximum(ii.max(), jj.max())) + 1 if ii.numel() else t0
        E = ii.numel()
        P = patches.reshape(1, -1, *patches.shape[-3:])
        for _ in range(iterations):
            cur, new_patches = BA(cur, P, K, target.reshape(1, E, 2), weight.reshape(1, E, 2), lmbda,
                                  ii, jj, kk, bounds, ep=100.0, fixedp=t0,
                                  structure_only=(t1 - t0 == 0), num_poses=n)
            patches.copy_(new_patches.view(patches.shape))
            P = patches.reshape(1, -1, *patches.shape[-3:])
        out = cur.data.view(shape)
        if not is_group:
            pdata.copy_(out)
            return pdata
        return out


__all__ = ["CholeskySolver", "block_matmul", "block_solve", "BA", "python_ba_wrapper",
           "layer_status"]
