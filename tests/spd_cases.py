"""Shared by the SPD-solve tests (spd_solve.hip through cuda_ba.spd_solve /
spd_solve_factored): the launch rule restated, matrices of a chosen condition
number, constructed failures, backward errors in numpy.longdouble, and the
reference (torch.linalg.cholesky_ex + torch.cholesky_solve on the CPU, in the
case's own dtype, on the same rounded inputs).

    solve:   eta = ||H x - b||_F / (||H||_F ||x||_F + ||b||_F)
    factor:  phi = ||L L^T - H||_F / ||H||_F
    bars:    eta_gpu <= 4 max(eta_ref, u),  phi_gpu <= 8 max(phi_ref, u)

with H the symmetric matrix that the lower triangle defines and u the unit
roundoff of the dtype.  The margins: a NumPy restatement of the kernel's
algorithm (unblocked, right-looking, reciprocal-multiply sweeps, no FMA)
against LAPACK gave at most 0.94 x LAPACK's eta and 3.72 x its phi (n = 257,
fp64, cond 10; the unblocked factor's residual grows faster with n than the
blocked one's).  4 x is the margin over a same-rounding-model reference in
test_update_op_gpu.py and test_encoder_gpu.py; the factor gets 8 x for the
3.72.
"""
import functools
import json
import sys
import time

import numpy as np
import torch

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the backward errors need an 80-bit long double"

F32, F64 = torch.float32, torch.float64
LDS, RAISED, HBM = "lds", "lds>64K", "hbm"
ETA_MARGIN, PHI_MARGIN = 4.0, 8.0
MAX_N_F64 = 8184  # DPVO_SPD_MAX_N_F64: (64 KB - 64 B) / 8, = 6 x 1364 free poses of the BA layer


def unit_roundoff(dtype):
    return torch.finfo(dtype).eps / 2


def residency(n, k, dtype):
    """spd_launch's rule: where the working matrix of an (n, k) call lives."""
    size = torch.finfo(dtype).bits // 8
    nbytes = size * (n * n + n * k + n)
    if nbytes <= 160 * 1024 - 64:
        return RAISED if nbytes > 64 * 1024 else LDS
    return HBM


# (dtype, n, k, residency); each at both condition numbers of its dtype
CONDS = {F64: (10.0, 1e10), F32: (10.0, 1e4)}
SIZES = [(F64, 1, 1, LDS), (F64, 2, 1, LDS), (F64, 33, 1, LDS), (F64, 34, 1, LDS), (F64, 65, 1, LDS),
         (F64, 66, 1, LDS), (F64, 89, 1, LDS), (F64, 90, 1, RAISED), (F64, 142, 1, RAISED),
         (F64, 143, 1, HBM), (F64, 258, 1, HBM), (F64, 300, 1, HBM),
         (F32, 1, 1, LDS), (F32, 2, 1, LDS), (F32, 33, 1, LDS), (F32, 65, 1, LDS), (F32, 127, 1, LDS),
         (F32, 128, 1, RAISED), (F32, 201, 1, RAISED), (F32, 202, 1, HBM), (F32, 258, 1, HBM),
         (F32, 300, 1, HBM),
         (F32, 7, 3, LDS), (F32, 66, 2, LDS), (F32, 8, 257, LDS), (F32, 120, 300, HBM),
         # 8 (n^2 + 3 n) crosses 160 KB - 64 B between n = 141 and 142
         (F64, 140, 2, RAISED), (F64, 141, 2, RAISED), (F64, 142, 2, HBM), (F64, 257, 2, HBM)]
ACCURACY = [(dt, n, k, cond, res) for dt, n, k, res in SIZES for cond in CONDS[dt]]


def case_id(c):
    dt, n, k, cond = c[:4]
    return f"{'f64' if dt == F64 else 'f32'}-n{n}-k{k}-cond{cond:g}"


def spd(n, k, cond, dtype, seed=0, batch=1):
    """H [batch, n, n] = Q diag(lambda) Q^T, lambda log-spaced from 1 to
    1 / cond, Q from the QR of a seeded fp64 normal matrix; symmetrised, then
    rounded to dtype.  b [batch, n, k] seeded normal.  CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    lam = torch.logspace(0, -np.log10(cond), n, dtype=F64) if n > 1 else torch.ones(1, dtype=F64)
    Q = torch.linalg.qr(torch.randn(batch, n, n, generator=g, dtype=F64))[0]
    H = (Q * lam) @ Q.transpose(-1, -2)
    H = 0.5 * (H + H.transpose(-1, -2))
    b = torch.randn(batch, n, k, generator=g, dtype=F64)
    return H.to(dtype), b.to(dtype)


# ------------------------------------------------------------------ failures
KINDS = ("col0", "last", "nan_pivot", "nan_offdiag")


def break_at(H, kind):
    """A copy of the SPD matrix H [n, n] that fails, and where: (H', info,
    poisoned) with info the 1-based first failed column and poisoned = (row,
    first column) of the entries of L that a NaN below the diagonal reaches
    before that column (None for a broken pivot)."""
    n = H.shape[-1]
    H = H.clone()
    if kind == "col0":
        H[0, 0] = -1.0
        return H, 1, None
    if kind == "last":
        H[n - 1, n - 1] = -1.0
        return H, n, None
    if kind == "nan_pivot":
        j = n // 2
        H[j, j] = float("nan")
        return H, j + 1, None
    if kind == "nan_offdiag":
        i, j = (2 * n) // 3, n // 4
        assert i > j
        H[i, j] = float("nan")
        return H, i + 1, (i, j)
    raise KeyError(kind)


# ------------------------------------------------------------------ errors
def _ld(t):
    return t.detach().cpu().double().numpy().astype(LD)


def sym_lower(H):
    """longdouble [.., n, n]: the symmetric matrix the lower triangle defines."""
    A = np.tril(_ld(H))
    return A + np.swapaxes(np.tril(A, -1), -1, -2)


def _fro(a):
    return np.sqrt((a * a).sum(axis=(-1, -2)))


def eta(H, x, b):
    """Largest normwise backward error of the solves over the batch items."""
    A, x, b = sym_lower(H), _ld(x), _ld(b)
    r = _fro(A @ x - b) / (_fro(A) * _fro(x) + _fro(b))
    return float(np.max(r))


def phi(H, L):
    A, L = sym_lower(H), _ld(L)
    return float(np.max(_fro(L @ np.swapaxes(L, -1, -2) - A) / _fro(A)))


def reference_solve(H, b):
    """cholesky_ex + cholesky_solve on the CPU in H's dtype -> (x, L, info)."""
    L, info = torch.linalg.cholesky_ex(H)
    return torch.cholesky_solve(b, L), L, info


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's inputs and what the CPU reference makes of them."""
    dt, n, k, cond = case[:4]
    H, b = spd(n, k, cond, dt, seed=1000 * k + n)
    x, L, info = reference_solve(H, b)
    return {"H": H, "b": b, "x": x, "L": L, "info": info, "eta": eta(H, x, b), "phi": phi(H, L),
            "u": unit_roundoff(dt)}


def bars(ref):
    return ETA_MARGIN * max(ref["eta"], ref["u"]), PHI_MARGIN * max(ref["phi"], ref["u"])


# ------------------------------------------------------------------ the largest launch
BAND = 8


def band_factor(n, seed=0):
    """L = 2 I + a strictly lower band of width 8 with entries in [-0.1, 0.1]:
    -> (L dense fp64 [n, n], its diagonals as longdouble: ld[p][m] = L[m + p, m])."""
    g = torch.Generator().manual_seed(seed)
    L = torch.zeros(n, n, dtype=F64)
    L.diagonal().fill_(2.0)
    ld = [np.full(n, 2.0, LD)]
    for p in range(1, BAND + 1):
        v = 0.2 * torch.rand(n - p, generator=g, dtype=F64) - 0.1
        L.diagonal(-p).copy_(v)
        ld.append(v.numpy().astype(LD))
    return L, ld


def band_eta(ld, x, b):
    """eta of x for H = L L^T, all O(n) in longdouble from the diagonals of L."""
    n = len(ld[0])
    x, b = _ld(x).reshape(n), _ld(b).reshape(n)
    y = np.zeros(n, LD)  # L^T x
    for p, d in enumerate(ld):
        y[:n - p] += d * x[p:]
    Hx = np.zeros(n, LD)  # L y
    for p, d in enumerate(ld):
        Hx[p:] += d * y[:n - p]
    # ||H||_F: diagonal q of H, H[j + q, j] = sum_r L[j + q, j - r] L[j, j - r]
    h2 = LD(0)
    for q in range(BAND + 1):
        hq = np.zeros(n - q, LD)
        for r in range(BAND + 1 - q):
            m = n - q - r
            hq[r:] += ld[q + r][:m] * ld[r][:m]
        h2 += (1 if q == 0 else 2) * (hq * hq).sum()
    nrm = lambda v: np.sqrt((v * v).sum())  # noqa: E731
    return float(nrm(Hx - b) / (np.sqrt(h2) * nrm(x) + nrm(b)))


def largest_launch(n=MAX_N_F64):
    """A solve-only call at the largest n the BA layer admits (fp64, k = 1):
    eta of the device's x and of torch.cholesky_solve's, and the wall time of
    the device call."""
    from dpvo_amd.ba import _cuda_ba

    dev = torch.device("cuda:0")
    assert residency(n, 1, F64) == HBM
    L, ld = band_factor(n)
    b = torch.randn(n, 1, generator=torch.Generator().manual_seed(1), dtype=F64)
    ref = torch.cholesky_solve(b, L)
    Ld, bd = L.to(dev)[None], b.to(dev)[None]
    torch.cuda.synchronize()
    t = time.perf_counter()
    x = _cuda_ba.spd_solve_factored(Ld, bd)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t
    unchanged = bool(torch.equal(Ld[0].cpu(), L))
    return {"n": n, "eta_gpu": band_eta(ld, x[0], b), "eta_ref": band_eta(ld, ref, b),
            "seconds": seconds, "factor_unchanged": unchanged}


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(largest_launch()))
