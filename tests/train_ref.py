"""fp64 torch restatements (CPU) of the three pieces csrc/train.hip fuses:
projective_ops.transform (projective_ops.py:53-113), the flow loss of
train.py:87-88 and the pose loss of train.py:90-113.  Autograd differentiates
them.  Group elements are the 4x4 matrices of tests/se3_restatement.py; the
gradient of a pose is taken through the retraction Exp(e) G at e = 0, the
left-tangent row the kernels return.  Nothing here is shared with the kernels:
no quaternion algebra, no closed-form Jacobian, and the scale of the pose loss
comes from torch.linalg.svdvals.

Not a test file.
"""
import torch

import se3_restatement as L

F64 = torch.float64


def _retract(data):
    """SE3 data [n, 7] -> (e [n, 6] zero leaf, Exp(e) M [n, 4, 4])."""
    e = torch.zeros(data.shape[0], 6, dtype=F64, requires_grad=True)
    return e, L.Exp(e) @ L.from_data(data.to(F64))


def transform(poses, patches, intr, ii, jj, kk, g=None):
    """poses [N, 7], patches [M, 3, P, P], intr [N, 4], ii / jj / kk [E] (all
    in range) -> dict(coords [E, P, P, 2], valid [E, P, P], Z [E, P, P]) and,
    with a cotangent g of coords, g_poses [N, 6] and g_patches [M, 3, P, P]."""
    e, G = _retract(poses)
    K = patches.to(F64).clone().requires_grad_(True)
    intr = intr.to(F64)
    x, y, d = K[kk].unbind(1)  # [E, P, P]
    fx, fy, cx, cy = (intr[ii][:, c, None, None] for c in range(4))
    X0 = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(d), d], -1)
    Gij = G[jj] @ L.inv(G[ii])
    X1 = (Gij[:, None, None] @ X0[..., None])[..., 0]
    X, Y, Z = X1[..., 0], X1[..., 1], X1[..., 2]
    fx, fy, cx, cy = (intr[jj][:, c, None, None] for c in range(4))
    dinv = 1.0 / Z.clamp(min=0.1)
    coords = torch.stack([fx * (dinv * X) + cx, fy * (dinv * Y) + cy], -1)
    out = {"coords": coords.detach(), "valid": (Z > 0.2).to(F64).detach(), "Z": Z.detach()}
    if g is not None:
        gp, gk = torch.autograd.grad((coords * g.to(F64)).sum(), (e, K), allow_unused=True)
        out["g_poses"] = torch.zeros_like(e) if gp is None else gp
        out["g_patches"] = torch.zeros_like(K) if gk is None else gk
    return out


def flow_loss(x, y, valid, g=1.0):
    """x, y [E, P, P, 2], valid [E] -> dict(loss, count, emin [E], errors
    [E, P*P], g_coords): the mean over the valid edges of the minimum over the
    points of |x - y|; with no valid edge 0 and a zero gradient."""
    x = x.to(F64).clone().requires_grad_(True)
    err = (x - y.to(F64)).norm(dim=-1).reshape(x.shape[0], -1)
    emin = err.min(dim=-1).values
    ok = valid.reshape(-1) > 0.5
    n = int(ok.sum())
    loss = emin[ok].mean() if n else (emin * 0).sum()
    (gx,) = torch.autograd.grad(loss * g, x)
    return {"loss": loss.detach(), "count": n, "emin": emin.detach(), "errors": err.detach(),
            "g_coords": gx}


def pose_scale(G, Ps):
    """kabsch_umeyama(t_gt, t_est).clamp(max=10) of train.py:31-41, 102-105 on
    the translations of inv(Ps) and inv(G); singular values from svdvals."""
    A = L.inv(L.from_data(Ps.to(F64)))[:, :3, 3]
    B = L.inv(L.from_data(G.to(F64)))[:, :3, 3]
    n = A.shape[0]
    EA, EB = A.mean(0), B.mean(0)
    var = ((A - EA).norm(dim=1) ** 2).mean()
    H = ((A - EA).T @ (B - EB)) / n
    return (var / torch.linalg.svdvals(H).sum()).clamp(max=10.0)


def pose_loss(G, Ps, g_tr=1.0, g_ro=1.0):
    """G, Ps [n, 7] -> dict(tr, ro (means), tr_pairs, ro_pairs [n (n - 1)], s,
    g_G [n, 6]) of train.py:90-113."""
    n = G.shape[0]
    s = pose_scale(G, Ps).detach()
    e, M = _retract(G)
    P1 = L.inv(M)
    P1 = torch.cat([torch.cat([P1[:, :3, :3], P1[:, :3, 3:] * s], -1), P1[:, 3:]], -2)
    P2 = L.inv(L.from_data(Ps.to(F64)))
    ii, jj = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    k = ii != jj
    ii, jj = ii[k], jj[k]
    dP = L.inv(P1[ii]) @ P1[jj]
    dG = L.inv(P2[ii]) @ P2[jj]
    e1 = L.Log(dP @ L.inv(dG))
    # a pair of bitwise identical poses (in G and in Ps) has e = Log(I) = 0 and,
    # by the subgradient torch takes for |0|, a zero gradient; the matrix
    # inverse above would leave rounding noise with an arbitrary direction
    twin = (G[ii] == G[jj]).all(-1) & (Ps[ii] == Ps[jj]).all(-1)
    e1 = e1 * (~twin)[:, None].to(F64)
    tr, ro = e1[:, :3].norm(dim=-1), e1[:, 3:].norm(dim=-1)
    (gG,) = torch.autograd.grad(g_tr * tr.mean() + g_ro * ro.mean(), e)
    return {"tr": tr.mean().detach(), "ro": ro.mean().detach(), "tr_pairs": tr.detach(),
            "ro_pairs": ro.detach(), "s": s, "g_G": gG}
