"""The (theta, sigma) sweep of Sim3 (lietorch group 4) shared by
test_sim3_host.py (dpvo_amd/csrc/sim3.hpp compiled for the host),
test_sim3_bands_gpu.py (the kernels), test_sim3_restatement.py (the oracle
itself) and test_pgo_loop_gpu.py: inputs that walk the rotation angle and the
log-scale through every regime of sim3.hpp, the expected result of every
forward and backward op, and the error measure (lie_bands.row_error).

Regimes: w_coeffs switches at theta = 0.05 (kTheta2) and |sigma| = 0.5
(kSigma), four combinations; logm at theta ~ 0.02 (kLogR2), at w < 0 and
through w = 0.  The grid is the full product THETA x SIGMA with both sides of
each switch, 4 seeded random axes per point, tau ~ N(0, 1).

Elements are exact images of the known tangent a: t = Exp(a)[:3, 3] by the
restatement, q the half-angle closed form, s = e^sigma.  Every second row's
quaternion is negated (w < 0) and every second pair is scaled by 1.3
(normalised on load).

References.  f64: log is a itself; Jinv, log backward and exp backward come
from the left Jacobian J_l(a) (a linear solve of condition <= 14 over the
grid, regular through pi); everything else from the restatement at the
kernel's inputs.  f32: the inputs are rounded first and a' = R.Log of the
rounded element takes the place of a (the f32 angles stop at pi - 1e-3, where
R.Log is good to 1.4e-13).
"""
import functools
import math

import torch

import se3_restatement as SE3R
import sim3_restatement as R
from lie_bands import row_error, to_numpy  # noqa: F401  (re-exported)

F64 = torch.float64
PI = math.pi
THETA = [0.0, 1e-9, 1e-5, 1e-3, 0.0199, 0.0201, 0.0499, 0.0501, 0.3, 1.0, 2.0, 3.0, PI - 1e-3]
THETA_F64 = [PI - 1e-6]                      # f64 only
THETA_EXP = [PI + 1e-3, 4.0, 2 * PI - 0.1]   # tangents given to exp / exp backward only
SIGMA = [0.0, 1e-9, -1e-5, 1e-3, 0.1, -0.499, 0.499, 0.501, -0.501, 1.0, -2.0, 3.0]
PER_POINT = 4
BLOCK_N, BLOCK_POINT = 257, (0.0499, 0.501)  # the recurrence branch across the 256-thread block edge

K, N = 7, 8
FWD_OPS = ["exp", "log", "inv", "mul", "adj", "adjT", "act", "act4", "matrix", "projector", "Jinv"]
BWD_OPS = ["exp", "log", "inv", "mul", "adj", "adjT", "act", "act4"]
GROUP_VALUED = ("exp", "inv", "mul")
OP_INDEX = {op: i for i, op in enumerate(FWD_OPS)}  # the op numbers of sim3.hpp
GRAD_DIM = {"exp": N, "log": K, "inv": N, "mul": N, "adj": K, "adjT": K, "act": 3, "act4": 4}


def thetas_of(op, f64):
    return THETA + (THETA_F64 if f64 else []) + (THETA_EXP if op == "exp" else [])


def element(a, flip=True):
    """Sim3 data [n, 8] of Exp(a) for a tangent a [n, 7] of any angle."""
    n = len(a)
    theta = a[:, 3:6].norm(dim=1, keepdim=True)
    axis = torch.where(theta > 0, a[:, 3:6] / theta.clamp(min=1e-300), torch.zeros_like(a[:, 3:6]))
    q = torch.cat([torch.sin(theta / 2) * axis, torch.cos(theta / 2)], 1)
    if flip:
        i = torch.arange(n)
        sign = torch.where(i % 2 == 1, -1.0, 1.0).to(F64)
        scale = torch.where((i // 2) % 2 == 1, 1.3, 1.0).to(F64)
        q = q * (sign * scale)[:, None]
    return torch.cat([R.Exp(a)[:, :3, 3], q, torch.exp(a[:, 6:7])], 1)


def to_data(M):
    """[..., 4, 4] -> Sim3 data [..., 8], right for any rotation (the
    largest-component quaternion of se3_restatement.to_data)."""
    s = torch.linalg.det(M[..., :3, :3]) ** (1.0 / 3.0)
    E = M.clone()
    E[..., :3, :3] = M[..., :3, :3] / s[..., None, None]
    return torch.cat([SE3R.to_data(E), s[..., None]], -1)


def grid_tangents(thetas, per=PER_POINT, seed=40):
    """[len(thetas) * len(SIGMA) * per, 7]: (tau ~ N(0, 1), theta * axis, sigma)."""
    pts = [(t, s) for t in thetas for s in SIGMA]
    return tangents_at(pts, per, seed + len(thetas))


def tangents_at(pts, per, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(pts) * per
    theta = torch.tensor([p[0] for p in pts], dtype=F64).repeat_interleave(per)
    sigma = torch.tensor([p[1] for p in pts], dtype=F64).repeat_interleave(per)
    axis = torch.randn(n, 3, dtype=F64, generator=g)
    axis = axis / axis.norm(dim=1, keepdim=True)
    tau = torch.randn(n, 3, dtype=F64, generator=g)
    return torch.cat([tau, theta[:, None] * axis, sigma[:, None]], 1), g


@functools.lru_cache(maxsize=None)
def inputs(op, backward, f64, case):
    """(a [n, 7], x, y or None, grad or None) as fp64 CPU tensors: a is the
    tangent of every row, x the tangent (exp) or the element Exp(a)."""
    if case == "block":
        a, g = tangents_at([BLOCK_POINT], BLOCK_N, 7)
    else:
        a, g = grid_tangents(thetas_of(op, f64))
    n = len(a)
    x = a if op == "exp" else element(a)
    y = None
    if op == "mul":
        b = torch.randn(n, 7, dtype=F64, generator=g)
        b[:, 6] = 2 * torch.rand(n, dtype=F64, generator=g) - 1  # |sigma| <= 1
        y = element(b)
    elif op in ("adj", "adjT", "Jinv"):
        y = torch.randn(n, K, dtype=F64, generator=g)
    elif op in ("act", "act4"):
        y = torch.randn(n, 3 if op == "act" else 4, dtype=F64, generator=g)
    grad = torch.randn(n, GRAD_DIM[op], dtype=F64, generator=g) if backward else None
    return a, x, y, grad


def reference_fwd(op, a, x, y):
    """fp64 reference of a forward op; group-valued results as 4x4 matrices.
    `a` is Log of the element x as the caller knows it."""
    if op == "exp":
        return R.Exp(x)
    if op == "log":
        return a
    if op == "Jinv":
        return R.Jinv_solve(a, y)
    M = R.from_data(x)
    if op == "inv":
        return R.inv(M)
    if op == "mul":
        return M @ R.from_data(y)
    if op in ("adj", "adjT"):
        A = R.Adj_matrix(M)
        return ((A.transpose(-1, -2) if op == "adjT" else A) @ y[..., None])[..., 0]
    if op == "act":
        return R.act(M, y)
    if op == "act4":
        return R.act4(M, y)
    if op == "matrix":
        return M.reshape(-1, 16)
    if op == "projector":
        return R.projector(x).reshape(-1, 64)
    raise KeyError(op)


def reference_bwd(op, a, grad, x, y):
    """fp64 reference of a backward op: a tuple like lietorch_backends.*_backward."""
    if op == "exp":  # g^T J_l(x)
        return ((grad[:, None, :K] @ R.Jl(x))[:, 0],)
    if op == "log":  # J_l(a)^-T g
        sol = torch.linalg.solve(R.Jl(a).transpose(-1, -2), grad[..., None])[..., 0]
        return (torch.cat([sol, torch.zeros_like(sol[:, :1])], 1),)
    M = R.from_data(x)
    if op == "inv":
        return R.inv_backward(grad, M)
    if op == "mul":
        return R.mul_backward(grad, M, R.from_data(y))
    return {"adj": R.adj_backward, "adjT": R.adjT_backward, "act": R.act_backward,
            "act4": R.act4_backward}[op](grad, M, y)


@functools.lru_cache(maxsize=None)
def case(op, backward, dt, which):
    """(x, y, grad, reference) for the dtype `dt` ("f64" / "f32"): the inputs
    rounded to it (as fp64) and the reference at them."""
    a, x, y, g = inputs(op, backward, dt == "f64", which)
    if dt == "f32":
        r = lambda t: None if t is None else t.float().double()  # noqa: E731
        x, y, g = r(x), r(y), r(g)
        a = x if op == "exp" else R.Log(R.from_data(x))
    ref = reference_bwd(op, a, g, x, y) if backward else reference_fwd(op, a, x, y)
    return x, y, g, ref


def forward_error(op, out, ref):
    """(row error, | |q| - 1 | or 0) of a forward result `out` (fp64, native
    layout); group-valued results as matrices, so either quaternion sign passes."""
    if op in GROUP_VALUED:
        return row_error(R.from_data(out), ref), float((out[:, 3:7].norm(dim=1) - 1).abs().max())
    return row_error(out, ref), 0.0


def backward_error(outs, refs):
    assert len(outs) == len(refs)
    return max(row_error(o, r) for o, r in zip(outs, refs))
