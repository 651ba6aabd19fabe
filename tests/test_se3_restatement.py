"""CPU: tests/se3_restatement.py (matrix exponential + autograd) against the
closed forms of Exp, J_l and J_l^-1 of SE3 evaluated far beyond fp64: mpmath
at 60 digits when it can be imported, and always the theta^2 Taylor series of
the five coefficients (40 terms, summed exactly in rationals, which converges
for every angle used here).  The restatement is the reference of the 1e-10
sweeps, so it gets 1e-13 itself."""
from fractions import Fraction
from math import factorial

import numpy as np
import pytest
import torch

import se3_restatement as R

F64 = torch.float64
THETAS = [2e-6, 1e-4, 1e-2, 1.0, 3.0]
BOUND = 1e-13

try:
    import mpmath
except ImportError:  # the series below then stands alone
    mpmath = None


def _tangents(theta, n=4):
    g = torch.Generator().manual_seed(int(theta * 1e7) % 1000 + 1)
    axis = torch.randn(n, 3, dtype=F64, generator=g)
    axis = axis / axis.norm(dim=1, keepdim=True)
    return torch.cat([torch.randn(n, 3, dtype=F64, generator=g), theta * axis], 1)


# a = sin t / t, b = (1 - cos t) / t^2, c = (t - sin t) / t^3,
# d = (t^2 + 2 cos t - 2) / (2 t^4), e = (2 t - 3 sin t + t cos t) / (2 t^5)
def _coeffs_series(x):
    """Exact rational sums of the Taylor series in t^2 at the fp64 tangent x."""
    t2 = sum(Fraction(float(v)) ** 2 for v in x[3:])
    out = [Fraction(0)] * 5
    p = Fraction(1)
    for k in range(40):  # 9^40 / 81! < 1e-80
        s = (-1) ** k * p
        out[0] += s / factorial(2 * k + 1)
        out[1] += s / factorial(2 * k + 2)
        out[2] += s / factorial(2 * k + 3)
        out[3] += s / factorial(2 * k + 4)
        out[4] += s * (k + 1) / factorial(2 * k + 5)
        p *= t2
    one = 2 ** 300  # keep 90 digits: the matrix algebra that follows stays cheap
    return [Fraction(round(c * one), one) for c in out], Fraction


def _coeffs_mpmath(x):
    mpmath.mp.dps = 60
    mpf = mpmath.mpf
    t = mpmath.sqrt(sum(mpf(float(v)) ** 2 for v in x[3:]))
    s, c = mpmath.sin(t), mpmath.cos(t)
    return [s / t, (1 - c) / t ** 2, (t - s) / t ** 3, (t ** 2 + 2 * c - 2) / (2 * t ** 4),
            (2 * t - 3 * s + t * c) / (2 * t ** 5)], mpf


def _hat(v, zero):
    return [[zero, -v[2], v[1]], [v[2], zero, -v[0]], [-v[1], v[0], zero]]


def _mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))]
            for i in range(len(A))]


def _lin(terms, n=3):
    return [[sum(c * M[i][j] for c, M in terms) for j in range(n)] for i in range(n)]


def _solve(A, B):
    """Gauss-Jordan with partial pivoting in the scalar type of A."""
    n = len(A)
    M = [list(A[i]) + list(B[i]) for i in range(n)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(M[r][c]))
        M[c], M[p] = M[p], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


def _closed_forms(x, coeffs):
    """(Exp 4x4, J_l 6x6, J_l^-1 6x6) of one tangent as fp64 numpy arrays."""
    (a, b, c, d, e), num = coeffs(x)
    zero, one = num(0), num(1)
    v = [num(float(u)) for u in x]
    I3 = [[one if i == j else zero for j in range(3)] for i in range(3)]
    T, P = _hat(v[:3], zero), _hat(v[3:], zero)
    PP = _mm(P, P)
    Rm = _lin([(one, I3), (a, P), (b, PP)])
    V = _lin([(one, I3), (b, P), (c, PP)])
    PT, TP = _mm(P, T), _mm(T, P)
    PTP = _mm(PT, P)
    Q = _lin([(one / 2, T), (c, PT), (c, TP), (c, PTP), (d, _mm(P, PT)), (d, _mm(TP, P)),
              (-3 * d, PTP), (e, _mm(PTP, P)), (e, _mm(P, PTP))])
    t = [sum(V[i][k] * v[k] for k in range(3)) for i in range(3)]
    E = [Rm[i] + [t[i]] for i in range(3)] + [[zero, zero, zero, one]]
    J = [V[i] + Q[i] for i in range(3)] + [[zero] * 3 + V[i] for i in range(3)]
    I6 = [[one if i == j else zero for j in range(6)] for i in range(6)]
    Ji = _solve(J, I6)
    f = lambda M: np.array([[float(u) for u in row] for row in M])  # noqa: E731
    return f(E), f(J), f(Ji)


def _check(theta, coeffs):
    x = _tangents(theta)
    E, J, Ji = R.Exp(x), R.Jl(x), R.Jl_inv(x)
    errs = {"Exp": 0.0, "Jl": 0.0, "Jl_inv": 0.0}
    for n in range(len(x)):
        rE, rJ, rJi = _closed_forms(x[n].tolist(), coeffs)
        for name, got, ref in (("Exp", E[n], rE), ("Jl", J[n], rJ), ("Jl_inv", Ji[n], rJi)):
            e = np.abs(got.numpy() - ref) / np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
            errs[name] = max(errs[name], float(e.max()))
    print(f"theta={theta:g} {errs}")
    assert all(v <= BOUND for v in errs.values()), (theta, errs)


@pytest.mark.parametrize("theta", THETAS)
def test_restatement_matches_series(theta):
    _check(theta, _coeffs_series)


@pytest.mark.parametrize("theta", THETAS)
def test_restatement_matches_mpmath(theta):
    # without mpmath the exact series is the check (never a skip)
    _check(theta, _coeffs_mpmath if mpmath is not None else _coeffs_series)


def test_log_inverts_exp_at_every_angle():
    """Log (sim3_restatement's away from pi, the symmetric-part axis near it)
    and to_data (largest-component quaternion) round-trip through Exp."""
    for theta in (0.0, 1e-9, 2e-6, 1e-3, 0.3, 2.0, 3.0, np.pi - 1e-3, np.pi - 1e-6):
        x = _tangents(theta + 0.0)
        M = R.Exp(x)
        assert float((R.Log(M) - x).abs().max()) <= 1e-13 * max(1.0, float(x.abs().max())), theta
        back = R.from_data(R.to_data(M))
        assert float((back - M).abs().max()) <= 1e-14 * max(1.0, float(M.abs().max())), theta
