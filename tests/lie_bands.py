"""The angle sweep of SO3 / SE3 shared by test_lie_bands_gpu.py (the HIP
kernels) and test_oracle_lie_bands.py (the C oracle): inputs whose rotation
angle walks through every regime of the coefficient functions, the expected
result of every forward and backward op from tests/se3_restatement.py, and
the error measure.

Rows: 8 seeded random axes per angle, tau and every second operand ~ N(0, 1).
Group elements are Exp of these tangents by the restatement in fp64; every
second quaternion is negated (w < 0) and every second pair is scaled by 1.3
(normalised on load).  SO3 is the rotation part of the same rows.
"""
import functools
import math

import numpy as np
import torch

import se3_restatement as R

F64 = torch.float64
PI = math.pi
ANGLES = [0.0, 1e-9, 5e-7, 9.9e-7, 1.01e-6, 2e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 5e-2, 0.3,
          1.0, 2.0, 3.0, PI - 1e-3]
ANGLES_F64 = [PI - 1e-6]          # f64 only
ANGLES_EXP = [4.0, 2 * PI - 0.1, 7.0]  # tangents given to exp / exp backward only
NEAR_PI = 1e-3                    # within this of pi, log is checked by the round trip
PER_ANGLE = 8
BLOCK_N, BLOCK_ANGLE = 257, 1e-4  # one case across the 256-thread block edge

DIMS = {1: (3, 4), 3: (6, 7)}     # group -> (K, N)
FWD_OPS = ["exp", "log", "inv", "mul", "adj", "adjT", "act", "act4", "matrix", "projector", "Jinv"]
BWD_OPS = ["exp", "log", "inv", "mul", "adj", "adjT", "act", "act4"]
GROUP_VALUED = ("exp", "inv", "mul")


def _grad_dim(group, op):
    K, N = DIMS[group]
    return {"exp": N, "log": K, "inv": N, "mul": N, "adj": K, "adjT": K, "act": 3, "act4": 4}[op]


def angles_of(op, f64, case):
    if case == "block":
        return [BLOCK_ANGLE]
    return ANGLES + (ANGLES_F64 if f64 else []) + (ANGLES_EXP if op == "exp" else [])


@functools.lru_cache(maxsize=None)
def inputs(group, op, backward, f64, case):
    """(theta [n], x, y or None, grad or None) as fp64 CPU tensors, SE3 or SO3
    layout.  The same rows for every op of a (dtype, case)."""
    angles = angles_of(op, f64, case)
    per = BLOCK_N if case == "block" else PER_ANGLE
    n = len(angles) * per
    g = torch.Generator().manual_seed(20 + len(angles))
    theta = torch.tensor(angles, dtype=F64).repeat_interleave(per)
    axis = torch.randn(n, 3, dtype=F64, generator=g)
    axis = axis / axis.norm(dim=1, keepdim=True)
    tang = torch.cat([torch.randn(n, 3, dtype=F64, generator=g), theta[:, None] * axis], 1)
    K, N = DIMS[group]

    def element(t):
        d = R.to_data(R.Exp(t))
        i = torch.arange(n)
        sign = torch.where(d[:, 6] < 0, -1.0, 1.0).to(F64)          # w > 0 first
        sign = sign * torch.where(i % 2 == 1, -1.0, 1.0).to(F64)    # then w < 0 on odd rows
        scale = torch.where((i // 2) % 2 == 1, 1.3, 1.0).to(F64)
        d = torch.cat([d[:, :3], d[:, 3:] * (sign * scale)[:, None]], 1)
        return d if group == 3 else d[:, 3:].contiguous()

    x = (tang if group == 3 else tang[:, 3:].contiguous()) if op == "exp" else element(tang)
    y = None
    if op == "mul":
        y = element(torch.randn(n, 6, dtype=F64, generator=g))
    elif op in ("adj", "adjT", "Jinv"):
        y = torch.randn(n, K, dtype=F64, generator=g)
    elif op in ("act", "act4"):
        y = torch.randn(n, 3 if op == "act" else 4, dtype=F64, generator=g)
    grad = torch.randn(n, _grad_dim(group, op), dtype=F64, generator=g) if backward else None
    return theta, x, y, grad


# ---- SO3 rides on SE3 with zero translation ----
def _tan6(group, a):
    return a if group == 3 else torch.cat([torch.zeros_like(a), a], -1)


def _data7(group, d):
    return d if group == 3 else torch.cat([torch.zeros_like(d[..., :3]), d], -1)


def _tan_out(group, a, padded=False):
    """[n, 6 (+1)] of the SE3 reference -> the group's own tangent layout."""
    if group == 3:
        return a
    return torch.cat([a[..., 3:6], a[..., 6:]], -1) if padded else a[..., 3:6]


def as_matrix(group, d):
    """Group data (either quaternion sign, any norm) -> 4x4."""
    return R.from_data(_data7(group, d))


def reference_fwd(group, op, x, y):
    """fp64 reference of a forward op; group-valued results as 4x4 matrices."""
    if op == "exp":
        return R.Exp(_tan6(group, x))
    M = as_matrix(group, x)
    if op == "log":
        return _tan_out(group, R.Log(M))
    if op == "inv":
        return R.inv(M)
    if op == "mul":
        return R.mul(M, as_matrix(group, y))
    if op in ("adj", "adjT"):
        A = R.Adj(M)
        A = A.transpose(-1, -2) if op == "adjT" else A
        return _tan_out(group, (A @ _tan6(group, y)[..., None])[..., 0])
    if op == "act":
        return R.act(M, y)
    if op == "act4":
        return R.act4(M, y)
    if op == "matrix":
        return R.matrix(M).reshape(-1, 16)
    if op == "projector":
        d = _data7(group, x)
        # rows (t, q) and tangent columns (tau, phi) of the Sim3 projector at s = 1;
        # the last column of lietorch's N x N projector is 0
        P = R.S.projector(torch.cat([d, torch.ones_like(d[..., :1])], -1))[..., :7, :6]
        P = P if group == 3 else P[..., 3:, 3:]
        return torch.cat([P, torch.zeros_like(P[..., :1])], -1).reshape(len(x), -1)
    if op == "Jinv":
        return _tan_out(group, R.Jinv(M, _tan6(group, y)))
    raise KeyError(op)


def reference_bwd(group, op, grad, x, y):
    """fp64 reference of a backward op: a tuple like lietorch_backends.*_backward."""
    K, N = DIMS[group]
    if op == "exp":
        g = torch.cat([_tan6(group, grad[:, :K]), torch.zeros_like(grad[:, :1])], -1)
        return (_tan_out(group, R.exp_backward(g, _tan6(group, x))[0]),)
    M = as_matrix(group, x)
    if op == "log":
        return (_tan_out(group, R.log_backward(_tan6(group, grad), M)[0], True),)
    if op == "inv":
        return (_tan_out(group, R.inv_backward(_tan6(group, grad[:, :K]), M)[0], True),)
    if op == "mul":
        a, b = R.mul_backward(_tan6(group, grad[:, :K]), M, as_matrix(group, y))
        return _tan_out(group, a, True), _tan_out(group, b, True)
    if op in ("adj", "adjT"):
        f = R.adj_backward if op == "adj" else R.adjT_backward
        a, b = f(_tan6(group, grad), M, _tan6(group, y))
        return _tan_out(group, a, True), _tan_out(group, b)
    if op in ("act", "act4"):
        a, b = (R.act_backward if op == "act" else R.act4_backward)(grad, M, y)
        return _tan_out(group, a, True), b
    raise KeyError(op)


def row_error(got, ref):
    """max over rows and entries of |got - ref| / max(1, max |ref| of the row)."""
    got, ref = got.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    scale = ref.abs().max(dim=1, keepdim=True)[0].clamp(min=1.0)
    return float(((got - ref).abs() / scale).max())


def forward_error(group, op, theta, x, out, ref):
    """Error of a forward result `out` (fp64, the op's native layout)."""
    if op in GROUP_VALUED:  # up to the quaternion's sign: as matrices, and of unit norm
        q = out[:, -4:]
        return max(row_error(as_matrix(group, out), ref),
                   float((q.norm(dim=1) - 1).abs().max()))
    if op == "log":
        near = theta >= PI - NEAR_PI
        err = row_error(out[~near], ref[~near])
        if near.any():  # the axis is ill-conditioned here: Exp(log X) == X instead
            back = R.Exp(_tan6(group, out[near]))
            err = max(err, row_error(back, as_matrix(group, x[near])))
        return err
    return row_error(out, ref)


def to_numpy(*ts):
    return [None if t is None else np.ascontiguousarray(t.numpy()) for t in ts]
