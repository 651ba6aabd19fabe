"""Sim3 in fp64 torch on the CPU: the comparison oracle of the Sim3 / loop
closure tests (test_sim3_gpu.py, test_pgo_loop_gpu.py).

It shares no branch structure with the kernels (dpvo_amd/csrc/sim3.hpp):
group elements are 4x4 matrices [[sR, t], [0, 1]], Exp is
torch.linalg.matrix_exp of the 4x4 generator, W is a block of a 6x6 matrix
exponential, and Log takes (phi, sigma) from the matrix logarithm of the 3x3
block sR (power series near the identity, det / atan2 closed form away from
it) and tau = W^-1 t.  Everything is differentiable by autograd and finite at
sigma = 0, theta = 0.  Tangent order (tau, phi, sigma), data order
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


def _log3_series(A):
    """Matrix logarithm of A near the identity: sum_k (-1)^(k+1) (A - I)^k / k."""
    E = A - torch.eye(3, dtype=A.dtype)
    P, L = E, E.clone()
    for k in range(2, 40):  # 0.3^40 / 40 < 1e-22
        P = P @ E
        L = L + ((-1.0) ** (k + 1) / k) * P
    sigma = (L[..., 0, 0] + L[..., 1, 1] + L[..., 2, 2]) / 3
    phi = 0.5 * torch.stack([L[..., 2, 1] - L[..., 1, 2], L[..., 0, 2] - L[..., 2, 0],
                             L[..., 1, 0] - L[..., 0, 1]], -1)
    return phi, sigma


def _log3_closed(A):
    s = torch.linalg.det(A) ** (1.0 / 3.0)
    R = A / s[..., None, None]
    v = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0],
                           R[..., 1, 0] - R[..., 0, 1]], -1)  # sin(theta) axis
    n = v.norm(dim=-1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    theta = torch.atan2(n, c)
    return v * (theta / n)[..., None], torch.log(s)


def Log(M):
    """[..., 4, 4] -> [..., 7]."""
    shape = M.shape[:-2]
    M = M.reshape(-1, 4, 4)
    A = M[:, :3, :3]
    near = (A - torch.eye(3, dtype=M.dtype)).flatten(1).norm(dim=1) < 0.3
    phi = torch.zeros(M.shape[0], 3, dtype=M.dtype)
    sigma = torch.zeros(M.shape[0], dtype=M.dtype)
    if near.any():
        p, s = _log3_series(A[near])
        phi = phi.index_put((near.nonzero()[:, 0],), p)
        sigma = sigma.index_put((near.nonzero()[:, 0],), s)
    if (~near).any():
        p, s = _log3_closed(A[~near])
        phi = phi.index_put(((~near).nonzero()[:, 0],), p)
        sigma = sigma.index_put(((~near).nonzero()[:, 0],), s)
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
