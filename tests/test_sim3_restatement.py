"""CPU: tests/sim3_restatement.py, the oracle of every Sim3 test, over the
(theta, sigma) grid of tests/sim3_bands.py.

Log takes the scale out before it chooses between series and closed form, so
a pure scaling (theta = 0, |sigma| >= 0.19), which the earlier Log sent into a
division by sin(theta) = 0, is finite; the rows stay here as a named case.
Log(Exp(a)) == a and Jinv (autograd through Log) == solve(J_l(a)) hold to
1e-12 up to theta = 3; next to pi Log is held to 1e-9 (its own accuracy there:
1.4e-13 at pi - 1e-3, 1.3e-10 at pi - 1e-6, the axis from sin(theta) axis) and
Jinv is not used: the sweeps take J_l^-1 from the solve, which is regular
through pi.  The backward references are autograd; they are checked against
central differences at general rows.

Measured: Log(Exp(a)) - a 3e-15 and Jinv against the solve 1e-14 for theta <=
3; cond(J_l) <= 13.7 over the grid.
"""
import math

import pytest
import torch

import sim3_bands as B
import sim3_restatement as R

F64 = torch.float64


@pytest.fixture(scope="module")
def grid():
    a, _ = B.grid_tangents(B.THETA + B.THETA_F64)
    return a, a[:, 3:6].norm(dim=1)


def test_finite_on_the_whole_grid(grid):
    a, _ = grid
    X = B.element(a)
    M = R.from_data(X)
    y = torch.randn(len(a), 7, dtype=F64, generator=torch.Generator().manual_seed(1))
    assert torch.isfinite(R.Log(M)).all()
    assert torch.isfinite(R.Jinv(M, y)).all()
    assert torch.isfinite(R.Jl(a)).all()
    # either quaternion sign and any norm give the same matrix as Exp
    assert B.row_error(M, R.Exp(a)) <= 1e-14


def test_pure_scale_rows():
    """theta = 0 exactly with |sigma| from 0.19 up: NaN before the repair."""
    sig = torch.tensor([0.19, 0.3, -0.499, 0.499, 0.501, -0.501, 1.0, -2.0, 3.0], dtype=F64)
    a = torch.zeros(len(sig), 7, dtype=F64)
    a[:, :3] = torch.randn(len(sig), 3, dtype=F64, generator=torch.Generator().manual_seed(2))
    a[:, 6] = sig
    M = R.Exp(a)
    assert float((R.Log(M) - a).abs().max()) <= 1e-12
    y = torch.randn(len(sig), 7, dtype=F64, generator=torch.Generator().manual_seed(3))
    J = R.Jinv(M, y)
    assert torch.isfinite(J).all()
    assert B.row_error(J, R.Jinv_solve(a, y)) <= 1e-12
    z = torch.zeros_like(a)
    Ji, Jj = R.pgo_jacobians(M, z, z)
    assert torch.isfinite(Ji).all() and torch.isfinite(Jj).all()


def test_log_inverts_exp(grid):
    a, theta = grid
    X = B.element(a)
    got = R.Log(R.from_data(X))
    low = theta <= 3.0 + 1e-9
    err = B.row_error(got[low], a[low])
    near = B.row_error(got[~low], a[~low])
    print(f"Log(Exp(a)) - a: theta <= 3 {err:.2e}, near pi {near:.2e}")
    assert err <= 1e-12
    assert near <= 1e-9
    assert int((~low).sum()) == 2 * len(B.SIGMA) * B.PER_POINT


def test_jinv_matches_the_solve(grid):
    a, theta = grid
    low = theta <= 3.0 + 1e-9
    a = a[low]
    y = torch.randn(len(a), 7, dtype=F64, generator=torch.Generator().manual_seed(4))
    J = R.Jl(a)
    cond = float(torch.linalg.cond(J).max())
    err = B.row_error(R.Jinv(R.from_data(B.element(a)), y), R.Jinv_solve(a, y))
    print(f"Jinv vs solve(J_l): {err:.2e}, cond(J_l) <= {cond:.1f}")
    assert err <= 1e-12


def test_left_jacobian_is_well_conditioned_through_pi(grid):
    """The near-pi references of the sweeps are solves with J_l: its condition
    number bounds what they lose (eigenvalues (e^z - 1) / z at z = sigma,
    sigma +- i theta, all away from 0 for theta < 2 pi)."""
    a, _ = grid
    cond = float(torch.linalg.cond(R.Jl(a)).max())
    print(f"cond(J_l) over the grid <= {cond:.2f}")
    assert cond <= 20.0
    # J_l against central differences of Exp, near pi
    x = a[-8:]
    J = R.Jl(x)
    h = 1e-6
    Ei = R.inv(R.Exp(x))
    for k in range(7):
        d = torch.zeros(7, dtype=F64)
        d[k] = h
        fd = R.vee((R.Exp(x + d) - R.Exp(x - d)) / (2 * h) @ Ei)
        assert float((fd - J[..., k]).abs().max()) <= 1e-7 * max(1.0, float(J.abs().max()))


def test_to_data_is_right_for_any_rotation():
    a, _ = B.grid_tangents(B.THETA + B.THETA_F64 + B.THETA_EXP)
    M = R.Exp(a)
    back = R.from_data(B.to_data(M))
    assert B.row_error(back, M) <= 1e-14


# ---- the backward references against central differences ----
def _general_rows(n=5, seed=5):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, 7, dtype=F64, generator=g)
    a[:, 3:6] *= 0.8
    a[:, 6] *= 0.5
    a[0, 3:6] = 0      # a pure scaling
    a[0, 6] = 0.7
    return a, g


def _central(F, n, dim, h=1e-6):
    """d F / d v at v = 0 for F: [n, dim] -> [n] (rows independent)."""
    cols = []
    for k in range(dim):
        d = torch.zeros(n, dim, dtype=F64)
        d[:, k] = h
        cols.append((F(d) - F(-d)) / (2 * h))
    return torch.stack(cols, -1)


def _tangent_of(Z, Z0):
    return R.Log(Z @ R.inv(Z0))


FD_TOL = 1e-8  # h^2 = 1e-12 truncation, 1e-16 / h = 1e-10 roundoff, values of order 10


@pytest.mark.parametrize("op", B.BWD_OPS)
def test_backward_references_match_central_differences(op):
    a, gen = _general_rows()
    n = len(a)
    M = R.Exp(a)
    g = torch.randn(n, B.GRAD_DIM[op], dtype=F64, generator=gen)
    dot = lambda u, v: (u * v).sum(-1)  # noqa: E731
    if op == "exp":
        got, = R.exp_backward(g, a)
        fd = _central(lambda d: dot(g[:, :7], _tangent_of(R.Exp(a + d), M)), n, 7)
        refs, gots = [fd], [got]
    elif op == "log":
        got, = R.log_backward(g, M)
        fd = _central(lambda d: dot(g, R.Log(R.Exp(d) @ M)), n, 7)
        refs, gots = [fd], [got[:, :7]]
        assert float(got[:, 7].abs().max()) == 0
    elif op == "inv":
        got, = R.inv_backward(g, M)
        Z0 = R.inv(M)
        fd = _central(lambda d: dot(g[:, :7], _tangent_of(R.inv(R.Exp(d) @ M), Z0)), n, 7)
        refs, gots = [fd], [got[:, :7]]
    elif op == "mul":
        b, _ = _general_rows(seed=6)
        Y = R.Exp(b)
        gx, gy = R.mul_backward(g, M, Y)
        Z0 = M @ Y
        fx = _central(lambda d: dot(g[:, :7], _tangent_of(R.Exp(d) @ M @ Y, Z0)), n, 7)
        fy = _central(lambda d: dot(g[:, :7], _tangent_of(M @ R.Exp(d) @ Y, Z0)), n, 7)
        refs, gots = [fx, fy], [gx[:, :7], gy[:, :7]]
    else:
        dim = {"adj": 7, "adjT": 7, "act": 3, "act4": 4}[op]
        y = torch.randn(n, dim, dtype=F64, generator=gen)
        if op in ("adj", "adjT"):
            tr = op == "adjT"
            f = lambda X, v: ((R.Adj_matrix(X).transpose(-1, -2) if tr else R.Adj_matrix(X))  # noqa: E731
                              @ v[..., None])[..., 0]
        else:
            f = R.act if op == "act" else R.act4
        gx, gy = getattr(R, op + "_backward")(g, M, y)
        fx = _central(lambda d: dot(g, f(R.Exp(d) @ M, y)), n, 7)
        fy = _central(lambda d: dot(g, f(M, y + d)), n, dim)
        refs, gots = [fx, fy], [gx[:, :7], gy]
        assert float(gx[:, 7].abs().max()) == 0
    for got, ref in zip(gots, refs):
        assert torch.isfinite(got).all()
        err = B.row_error(got, ref)
        print(f"{op}: autograd vs central differences {err:.2e}")
        assert err <= FD_TOL


def test_grid_has_every_regime():
    """Both sides of theta = 0.05, theta ~ 0.02 and |sigma| = 0.5, and the
    row counts the sweeps are sized by."""
    assert len(B.inputs("log", False, True, "sweep")[0]) == 672
    assert len(B.inputs("exp", False, True, "sweep")[0]) == 816
    t2 = [t * t for t in B.THETA]
    assert any(0 < v < 2.5e-3 for v in t2) and min(abs(math.sqrt(v) - 0.05) for v in t2) < 2e-4
    assert {s for s in B.SIGMA if abs(abs(s) - 0.5) < 2e-3} == {-0.499, 0.499, 0.501, -0.501}
    x = B.inputs("log", False, True, "sweep")[1]
    assert bool((x[1::2, 6] <= 0).all()) and bool((x[0::2, 6] >= 0).all())  # w < 0 on odd rows
