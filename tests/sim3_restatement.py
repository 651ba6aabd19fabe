"""Sim3 in fp64 torch on the CPU: the comparison oracle of the Sim3 / loop
closure tests (test_sim3_gpu.py, test_pgo_loop_gpu.py).

It shares no branch structure with the kernels (dpvo_amd/csrc/sim3.hpp):
group elements are 4x4 matrices [[sR, t], [0, 1]], Exp is
torch.linalg.matrix_exp of the 4x4 generator, W is a block of a 6x6 matrix
exponential, and Log takes sigma from det(sR), phi from the matrix logarithm
of the rotation R (power series near the identity, atan2 closed form away
from it) and tau = W^-1 t.  Everything is differentiable by autograd and
finite at sigma = 0 and at theta = 0, together or apart.  The left Jacobian
J_l is the derivative of the matrix exponential and regular through pi; every
backward op is autograd through these functions with the retraction Exp(e) X
(tests/test_sim3_restatement.py holds all of it to account).  Tangent order (tau, phi, sigma), data order
(tx, ty, tz, qx, qy, qz, qw, s) as in lietorch.
"""
import torch

F64 = torch.float64


def hat3(phi):
    o = torch.zeros_like(phi[..., 0])
    x, y, z = phi.unbind(-1)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(phi.shape[:-1] + (3, 3))


def hat(x):
    """[..., 7] -> [..., 4, 4] generator [[Phi + sigma I, tau], [0, 0]]."""
    top = hat3(x[..., 3:6]) + x[..., 6, None, None] * torch.eye(3, dtype=x.dtype)
    top = torch.cat([top, x[..., :3, None]], -1)
    return torch.cat([top, torch.zeros_like(top[..., :1, :])], -2)


def vee(M):
    """Inverse of hat for a matrix of the generator's form."""
    A = M[..., :3, :3]
    sigma = (A[..., 0, 0] + A[..., 1, 1] + A[..., 2, 2]) / 3
    phi = 0.5 * torch.stack([A[..., 2, 1] - A[..., 1, 2], A[..., 0, 2] - A[..., 2, 0],
                             A[..., 1, 0] - A[..., 0, 1]], -1)
    return torch.cat([M[..., :3, 3], phi, sigma[..., None]], -1)


def Exp(x):
    return torch.linalg.matrix_exp(hat(x))


def W_of(phi, sigma):
    """Top-right 3x3 block of matrix_exp([[Phi + sigma I, I], [0, 0]])."""
    A = hat3(phi) + sigma[..., None, None] * torch.eye(3, dtype=phi.dtype)
    top = torch.cat([A, torch.eye(3, dtype=phi.dtype).expand_as(A)], -1)
    M = torch.cat([top, torch.zeros_like(top)], -2)
    return torch.linalg.matrix_exp(M)[..., :3, 3:]


def _vee3(L):
    return 0.5 * torch.stack([L[..., 2, 1] - L[..., 1, 2], L[..., 0, 2] - L[..., 2, 0],
                             L[..., 1, 0] - L[..., 0, 1]], -1)


def _log3_series(Rm):
    """phi of a rotation near the identity: log R = sum_k (-1)^(k+1) (R - I)^k / k."""
    E = Rm - torch.eye(3, dtype=Rm.dtype)
    P, L = E, E.clone()
    for k in range(2, 40):  # 0.3^40 / 40 < 1e-22
        P = P @ E
        L = L + ((-1.0) ** (k + 1) / k) * P
    return _vee3(L)


def _log3_closed(Rm):
    v = _vee3(Rm)  # sin(theta) axis, theta >= 0.2 here
    n = v.norm(dim=-1)
    c = 0.5 * (Rm[..., 0, 0] + Rm[..., 1, 1] + Rm[..., 2, 2] - 1)
    theta = torch.atan2(n, c)
    return v * (theta / n)[..., None]


def Log(M):
    """[..., 4, 4] -> [..., 7].  The scale comes out first (s = det(sR)^(1/3),
    sigma = log s), so that the choice between series and closed form depends
    on the rotation alone: a pure scaling (theta = 0, any sigma) takes the
    series, which is regular there."""
    shape = M.shape[:-2]
    M = M.reshape(-1, 4, 4)
    s = torch.linalg.det(M[:, :3, :3]) ** (1.0 / 3.0)
    Rm = M[:, :3, :3] / s[:, None, None]
    sigma = torch.log(s)
    near = (Rm - torch.eye(3, dtype=M.dtype)).flatten(1).norm(dim=1) < 0.3
    phi = torch.zeros(M.shape[0], 3, dtype=M.dtype)
    if near.any():
        phi = phi.index_put((near.nonzero()[:, 0],), _log3_series(Rm[near]))
    if (~near).any():
        phi = phi.index_put(((~near).nonzero()[:, 0],), _log3_closed(Rm[~near]))
    tau = torch.linalg.solve(W_of(phi, sigma), M[:, :3, 3])
    return torch.cat([tau, phi, sigma[:, None]], -1).reshape(shape + (7,))


def rotmat(q):
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
                       -1).reshape(q.shape[:-1] + (3, 3))


def from_data(d):
    """Sim3 data [..., 8] (or SE3 data [..., 7], scale 1) -> [..., 4, 4]."""
    d = d.to(F64)
    s = d[..., 7] if d.shape[-1] == 8 else torch.ones_like(d[..., 0])
    top = torch.cat([s[..., None, None] * rotmat(d[..., 3:7]), d[..., :3, None]], -1)
    bot = torch.zeros_like(top[..., :1, :]) + torch.tensor([0, 0, 0, 1.0], dtype=F64)
    return torch.cat([top, bot], -2)


def to_data(M):
    """[..., 4, 4] -> data [..., 8] with qw > 0 (rotation angles below pi)."""
    A = M[..., :3, :3]
    s = torch.linalg.det(A) ** (1.0 / 3.0)
    R = A / s[..., None, None]
    w = 0.5 * torch.sqrt(1 + R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2])
    v = torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0],
                     R[..., 1, 0] - R[..., 0, 1]], -1) / (4 * w[..., None])
    return torch.cat([M[..., :3, 3], v, w[..., None], s[..., None]], -1)


def inv(M):
    return torch.linalg.inv(M)


def Adj_matrix(M):
    """[..., 7, 7]: column k is vee(M hat(e_k) M^-1)."""
    E = hat(torch.eye(7, dtype=F64))  # [7, 4, 4]
    cols = vee(M[..., None, :, :] @ E @ inv(M)[..., None, :, :])  # [..., k, 7]
    return cols.transpose(-1, -2)


def projector(d):
    """The 8x8 d(data) / d(left tangent) of sim3.h:79-87 (its last column is 0)."""
    d = d.to(F64)
    t, q, s = d[..., :3], d[..., 3:7] / d[..., 3:7].norm(dim=-1, keepdim=True), d[..., 7]
    J = torch.zeros(d.shape[:-1] + (8, 8), dtype=F64)
    J[..., :3, :3] = torch.eye(3, dtype=F64)
    J[..., :3, 3:6] = hat3(-t)
    J[..., :3, 6] = t
    J[..., 3:6, 3:6] = 0.5 * (q[..., 3, None, None] * torch.eye(3, dtype=F64) + hat3(-q[..., :3]))
    J[..., 6, 3:6] = -0.5 * q[..., :3]
    J[..., 7, 6] = s
    return J


def Jinv(M, a):
    """J_l^-1(Log M) a = d/de Log(Exp(e a) M) at e = 0, by autograd."""
    f = lambda e: Log(Exp(e[..., None] * a) @ M)  # noqa: E731
    e0 = torch.zeros(a.shape[:-1], dtype=F64)
    return torch.autograd.functional.jvp(f, e0, torch.ones_like(e0))[1]


def pgo_residual(C, gi, gj):
    """Log(C Exp(gi) Exp(gj)^-1): C [r, 4, 4] matrices, gi / gj [r, 7]."""
    return Log(C @ Exp(gi) @ inv(Exp(gj)))


def pgo_jacobians(C, gi, gj):
    """d res / d gi, d res / d gj, both [r, 7 (residual), 7 (dof)]."""
    f = lambda a, b: pgo_residual(C, a, b).sum(0)  # noqa: E731
    Ji, Jj = torch.autograd.functional.jacobian(f, (gi, gj))
    return Ji.permute(1, 0, 2), Jj.permute(1, 0, 2)


# ---- the left Jacobian and the backward ops (the layout of sim3::bwd: the
# gradient of a group element is a left-perturbation tangent in the first 7
# entries of an 8-wide row, the 8th is 0) ----
def Jl(x):
    """Left Jacobian [..., 7, 7]: column k is vee(dExp(x)[e_k] Exp(x)^-1)."""
    Ei = inv(Exp(x))
    cols = []
    for k in range(7):
        e = torch.zeros_like(x)
        e[..., k] = 1.0
        cols.append(vee(torch.autograd.functional.jvp(Exp, x, e)[1] @ Ei))
    return torch.stack(cols, -1)


def Jinv_solve(x, y):
    """J_l^-1(x) y by a linear solve: accurate at every angle, near pi too,
    where autograd through Log (Jinv above) is not."""
    return torch.linalg.solve(Jl(x), y[..., None])[..., 0]


def _pad(t):
    return torch.cat([t, torch.zeros_like(t[..., :1])], -1)


def exp_backward(g, x):
    """g [n, 8] (left tangent of Exp(x)) -> d/dx [n, 7]."""
    x = x.clone().requires_grad_(True)
    E = Exp(x)
    (g[..., :7] * vee(E @ inv(E.detach()))).sum().backward()
    return (x.grad,)


def _retraction_grads(f, g, M, y=None, group_valued=False):
    """Gradients of <g, f(Exp(e) M, y)> at e = 0 with respect to e (and y).  A
    group-valued f is read through the left tangent of f(.) f(M, y)^-1."""
    e = torch.zeros(M.shape[:-2] + (7,), dtype=F64, requires_grad=True)
    args = [Exp(e) @ M]
    if y is not None:
        y = y.clone().requires_grad_(True)
        args.append(y)
    out = f(*args)
    if group_valued:
        out = vee(out @ inv(out.detach()))
        g = g[..., :7]
    (g * out).sum().backward()
    return (_pad(e.grad),) if y is None else (_pad(e.grad), y.grad)


def log_backward(g, M):
    return _retraction_grads(Log, g, M)


def inv_backward(g, M):
    return _retraction_grads(inv, g, M, group_valued=True)


def mul_backward(g, M, Y):
    """Y [n, 4, 4]; its gradient is the left tangent of Y, by Exp(f) Y."""
    e = torch.zeros(M.shape[:-2] + (7,), dtype=F64, requires_grad=True)
    f = torch.zeros(M.shape[:-2] + (7,), dtype=F64, requires_grad=True)
    Z = (Exp(e) @ M) @ (Exp(f) @ Y)
    (g[..., :7] * vee(Z @ inv(Z.detach()))).sum().backward()
    return _pad(e.grad), _pad(f.grad)


def act(M, p):
    return (M[..., :3, :3] @ p[..., None])[..., 0] + M[..., :3, 3]


def act4(M, p):
    return (M @ p[..., None])[..., 0]


def adj_backward(g, M, a):
    return _retraction_grads(lambda X, v: (Adj_matrix(X) @ v[..., None])[..., 0], g, M, a)


def adjT_backward(g, M, a):
    return _retraction_grads(lambda X, v: (Adj_matrix(X).transpose(-1, -2) @ v[..., None])[..., 0],
                             g, M, a)


def act_backward(g, M, p):
    return _retraction_grads(act, g, M, p)


def act4_backward(g, M, p):
    return _retraction_grads(act4, g, M, p)
