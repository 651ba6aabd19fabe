"""SE3 (and SO3, as SE3 with zero translation) in fp64 torch on the CPU: the
comparison oracle of the angle sweeps (test_lie_bands_gpu.py,
test_oracle_lie_bands.py).

It is tests/sim3_restatement.py at sigma = 0, s = 1: group elements are 4x4
matrices [[R, t], [0, 1]], Exp is torch.linalg.matrix_exp of the generator,
the left Jacobian is the derivative of that matrix exponential
(torch.autograd.functional.jvp), its inverse a linear solve, and every
backward op is autograd through these functions with the retraction
Exp(e) X.  No closed-form coefficient, no small-angle switch: nothing here is
shared with dpvo_amd/csrc/lie.hip or oracle/dpvo_oracle.c.

Tangent order (tau, phi), data order (tx, ty, tz, qx, qy, qz, qw) as in
lietorch.  Gradients follow the kernels' layout: the gradient of a group
element is a left-perturbation tangent in the first 6 entries of a 7-wide
row, the 7th is 0.
"""
import math

import torch

import sim3_restatement as S

F64 = S.F64


def lift(x):
    """[..., 6] SE3 tangent -> [..., 7] Sim3 tangent with sigma = 0."""
    return torch.cat([x, torch.zeros_like(x[..., :1])], -1)


def hat(x):
    return S.hat(lift(x))


def vee(M):
    return S.vee(M)[..., :6]


def Exp(x):
    """[..., 6] -> [..., 4, 4]."""
    return S.Exp(lift(x))


def from_data(d):
    """SE3 data [..., 7] (any quaternion norm or sign) -> [..., 4, 4]."""
    return S.from_data(d[..., :7])


def to_data(M):
    """[..., 4, 4] -> SE3 data [..., 7].  The quaternion is taken from the
    largest of (x, y, z, w) (Shepperd), so it is accurate at every angle, pi
    included; its overall sign is arbitrary."""
    Rm = M[..., :3, :3]
    d = Rm.diagonal(dim1=-2, dim2=-1)
    tr = d.sum(-1)
    four_sq = torch.cat([1 + 2 * d - tr[..., None], (1 + tr)[..., None]], -1)  # 4 q_i^2
    k = four_sq.argmax(-1)
    # 4 q_k q_j for every (k, j)
    x, y, z = four_sq[..., 0], four_sq[..., 1], four_sq[..., 2]
    xy, xz, yz = Rm[..., 1, 0] + Rm[..., 0, 1], Rm[..., 0, 2] + Rm[..., 2, 0], Rm[..., 2, 1] + Rm[..., 1, 2]
    xw, yw, zw = Rm[..., 2, 1] - Rm[..., 1, 2], Rm[..., 0, 2] - Rm[..., 2, 0], Rm[..., 1, 0] - Rm[..., 0, 1]
    rows = torch.stack([torch.stack([x, xy, xz, xw], -1), torch.stack([xy, y, yz, yw], -1),
                        torch.stack([xz, yz, z, zw], -1), torch.stack([xw, yw, zw, four_sq[..., 3]], -1)],
                       -2)
    q = torch.gather(rows, -2, k[..., None, None].expand(k.shape + (1, 4)))[..., 0, :]
    q = q / q.norm(dim=-1, keepdim=True)
    return torch.cat([M[..., :3, 3], q], -1)


def matrix(M):
    return M


def inv(M):
    return S.inv(M)


def mul(A, B):
    return A @ B


def act(M, p):
    return (M[..., :3, :3] @ p[..., None])[..., 0] + M[..., :3, 3]


def act4(M, p):
    return (M @ p[..., None])[..., 0]


def Adj(M):
    """[..., 6, 6]: column k is vee(M hat(e_k) M^-1)."""
    return S.Adj_matrix(M)[..., :6, :6]


def _log_near_pi(M):
    """Log for rotation angles close to pi, where the antisymmetric part of R
    (sin(theta) axis) is too small to give the axis.  The symmetric part is
    cos(theta) I + (1 - cos(theta)) axis axis^T: the axis is its largest
    column, its sign comes from the antisymmetric part, and theta =
    atan2(sin, cos) is well conditioned there."""
    Rm = M[:, :3, :3]
    v = 0.5 * torch.stack([Rm[:, 2, 1] - Rm[:, 1, 2], Rm[:, 0, 2] - Rm[:, 2, 0],
                           Rm[:, 1, 0] - Rm[:, 0, 1]], -1)  # sin(theta) axis
    c = 0.5 * (Rm[:, 0, 0] + Rm[:, 1, 1] + Rm[:, 2, 2] - 1)
    theta = torch.atan2(v.norm(dim=-1), c)
    B = 0.5 * (Rm + Rm.transpose(1, 2)) - c[:, None, None] * torch.eye(3, dtype=M.dtype)
    k = B.diagonal(dim1=1, dim2=2).argmax(dim=1)
    a = B[torch.arange(M.shape[0]), :, k]
    a = a / a.norm(dim=-1, keepdim=True)
    sgn = torch.where((a * v).sum(-1) < 0, -1.0, 1.0).to(M.dtype)
    phi = a * (sgn * theta)[:, None]
    tau = torch.linalg.solve(S.W_of(phi, torch.zeros_like(theta)), M[:, :3, 3])
    return torch.cat([tau, phi], -1)


def Log(M):
    """[..., 4, 4] -> [..., 6], rotation angle below pi."""
    shape = M.shape[:-2]
    M = M.reshape(-1, 4, 4)
    c = 0.5 * (M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2] - 1)
    far = c < math.cos(3.0)
    out = torch.zeros(M.shape[0], 6, dtype=M.dtype)
    if (~far).any():
        out = out.index_put(((~far).nonzero()[:, 0],), S.Log(M[~far])[:, :6])
    if far.any():
        out = out.index_put((far.nonzero()[:, 0],), _log_near_pi(M[far]))
    return out.reshape(shape + (6,))


def Jl(x):
    """Left Jacobian [..., 6, 6]: column k is vee(dExp(x)[e_k] Exp(x)^-1)."""
    Ei = inv(Exp(x))
    cols = []
    for k in range(6):
        e = torch.zeros_like(x)
        e[..., k] = 1.0
        dE = torch.autograd.functional.jvp(Exp, x, e)[1]
        cols.append(vee(dE @ Ei))
    return torch.stack(cols, -1)


def Jl_inv(x):
    J = Jl(x)
    return torch.linalg.solve(J, torch.eye(6, dtype=x.dtype).expand_as(J))


def Jinv(M, a):
    """J_l^-1(Log M) a."""
    return torch.linalg.solve(Jl(Log(M)), a[..., None])[..., 0]


def _pad(t):
    return torch.cat([t, torch.zeros_like(t[..., :1])], -1)


def exp_backward(g, x):
    """g [n, 7] (left tangent of Exp(x), 7-wide) -> d/dx [n, 6] = g^T J_l(x)."""
    return ((g[..., None, :6] @ Jl(x))[..., 0, :],)


def log_backward(g, M):
    """g [n, 6] -> left tangent of X, 7-wide: g^T J_l^-1(Log X)."""
    J = Jl(Log(M))
    return (_pad(torch.linalg.solve(J.transpose(-1, -2), g[..., None])[..., 0]),)


def _retraction_grads(f, g, M, y=None, group_valued=False):
    """Gradients of <g, f(Exp(e) M, y)> at e = 0 with respect to e (and y).  A
    group-valued f is read through the left tangent of f(.) f(M, y)^-1."""
    e = torch.zeros(M.shape[:-2] + (6,), dtype=F64, requires_grad=True)
    args = [Exp(e) @ M]
    if y is not None:
        y = y.clone().requires_grad_(True)
        args.append(y)
    out = f(*args)
    if group_valued:
        out = vee(out @ inv(out.detach()))
        g = g[..., :6]
    (g * out).sum().backward()
    return (_pad(e.grad),) if y is None else (_pad(e.grad), y.grad)


def inv_backward(g, M):
    return _retraction_grads(inv, g, M, group_valued=True)


def mul_backward(g, M, Y):
    """Y [n, 4, 4]; its gradient is the left tangent of Y, by Exp(e) Y."""
    e = torch.zeros(M.shape[:-2] + (6,), dtype=F64, requires_grad=True)
    f = torch.zeros(M.shape[:-2] + (6,), dtype=F64, requires_grad=True)
    Z = (Exp(e) @ M) @ (Exp(f) @ Y)
    (g[..., :6] * vee(Z @ inv(Z.detach()))).sum().backward()
    return _pad(e.grad), _pad(f.grad)


def adj_backward(g, M, a):
    return _retraction_grads(lambda X, v: (Adj(X) @ v[..., None])[..., 0], g, M, a)


def adjT_backward(g, M, a):
    return _retraction_grads(lambda X, v: (Adj(X).transpose(-1, -2) @ v[..., None])[..., 0],
                             g, M, a)


def act_backward(g, M, p):
    return _retraction_grads(act, g, M, p)


def act4_backward(g, M, p):
    return _retraction_grads(act4, g, M, p)
