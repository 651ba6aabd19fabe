"""CPU: the reference side of every condition test_spd_solve_gpu.py relies
on: the launch rule puts the boundary sizes on the sides spd_solve.hip's header
names, every accuracy case is one the reference factors, the matrices have
the condition number asked for, every constructed failure fails where it was
built to fail (cholesky_ex's info), and the banded O(n) backward error of the
largest-launch case equals the dense one."""
import numpy as np
import pytest
import torch

import spd_cases as S


def test_boundary_sizes_lie_on_their_sides():
    r = S.residency
    assert (r(89, 1, S.F64), r(90, 1, S.F64)) == (S.LDS, S.RAISED)
    assert (r(142, 1, S.F64), r(143, 1, S.F64)) == (S.RAISED, S.HBM)
    assert (r(127, 1, S.F32), r(128, 1, S.F32)) == (S.LDS, S.RAISED)
    assert (r(201, 1, S.F32), r(202, 1, S.F32)) == (S.RAISED, S.HBM)
    # the byte counts themselves, at the two limits
    assert 8 * (142 * 142 + 2 * 142) <= 160 * 1024 - 64 < 8 * (143 * 143 + 2 * 143)
    assert 4 * (127 * 127 + 2 * 127) <= 64 * 1024 < 4 * (128 * 128 + 2 * 128)
    assert r(S.MAX_N_F64, 1, S.F64) == S.HBM and 8 * S.MAX_N_F64 == 64 * 1024 - 64


def test_every_case_names_its_residency():
    for dt, n, k, res in S.SIZES:
        assert S.residency(n, k, dt) == res, (dt, n, k)
    seen = {(dt, res) for dt, _, _, res in S.SIZES}
    assert seen == {(dt, res) for dt in (S.F32, S.F64) for res in (S.LDS, S.RAISED, S.HBM)}
    assert len(set(S.ACCURACY)) == len(S.ACCURACY) == 2 * len(S.SIZES)


@pytest.mark.parametrize("case", S.ACCURACY, ids=S.case_id)
def test_reference_factors_every_accuracy_case(case):
    ref = S.reference(case)
    assert int(ref["info"].abs().sum()) == 0
    assert torch.isfinite(ref["x"]).all() and torch.isfinite(ref["L"]).all()
    # the reference is backward stable on the case: |H - L L^T| <= gamma_(n+1) |L| |L^T| and
    # |dH| <= gamma_(3n+1) |L| |L^T| for the solve (Higham, Accuracy and Stability, thm 10.3 /
    # 10.4), with || |L| |L^T| ||_F <= trace(H) <= sqrt(n) ||H||_F
    n = case[1]
    assert ref["eta"] <= (3 * n + 1) * n ** 0.5 * ref["u"], ref["eta"]
    assert ref["phi"] <= (n + 1) * n ** 0.5 * ref["u"], ref["phi"]
    assert S.reference(case) is ref  # computed once


@pytest.mark.parametrize("dtype,n,cond", [(S.F64, 2, 1e10), (S.F64, 66, 1e10), (S.F32, 65, 1e4),
                                          (S.F64, 1, 10.0)])
def test_condition_number_and_symmetry(dtype, n, cond):
    H, b = S.spd(n, 3, cond, dtype, seed=4, batch=2)
    assert H.shape == (2, n, n) and b.shape == (2, n, 3) and H.dtype == b.dtype == dtype
    assert torch.equal(H, H.transpose(-1, -2))
    assert not torch.equal(H[0], H[1]) or n == 1
    ev = torch.linalg.eigvalsh(H.double())
    want = cond if n > 1 else 1.0
    got = (ev[:, -1] / ev[:, 0])
    assert ((got / want - 1).abs() < 1e3 * cond * S.unit_roundoff(dtype) + 1e-12).all(), got
    again = S.spd(n, 3, cond, dtype, seed=4, batch=2)
    assert torch.equal(again[0], H) and torch.equal(again[1], b)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("dtype,n", [(S.F64, 40), (S.F64, 150), (S.F32, 210)])
def test_constructed_failures_fail_where_built(dtype, n, kind):
    H = S.spd(n, 1, 10.0, dtype, seed=n)[0][0]
    Hb, info, poisoned = S.break_at(H, kind)
    assert 1 <= info <= n
    assert int(torch.linalg.cholesky_ex(Hb).info) == info
    assert int(torch.linalg.cholesky_ex(H).info) == 0
    changed = (Hb != H) & ~(torch.isnan(Hb) & torch.isnan(H))
    assert int(changed.sum()) == 1
    if poisoned is not None:
        i, j = poisoned
        assert info == i + 1 and j < i and torch.isnan(Hb[i, j])


def test_the_four_kinds_cover_first_last_and_both_nans():
    n = 40
    H = S.spd(n, 1, 10.0, S.F64)[0][0]
    infos = {k: S.break_at(H, k)[1] for k in S.KINDS}
    assert infos["col0"] == 1 and infos["last"] == n
    assert 1 < infos["nan_pivot"] < infos["nan_offdiag"] < n


def test_errors_are_zero_on_exact_data_and_see_a_perturbation():
    H = torch.tensor([[[4.0, 99.0], [2.0, 5.0]]], dtype=S.F64)  # the upper 99 is not read
    L = torch.tensor([[[2.0, 0.0], [1.0, 2.0]]], dtype=S.F64)
    x = torch.tensor([[[1.0], [2.0]]], dtype=S.F64)
    b = torch.tensor([[[8.0], [12.0]]], dtype=S.F64)
    assert S.phi(H, L) == 0.0 and S.eta(H, x, b) == 0.0
    assert 1e-9 < S.eta(H, x * (1 + 1e-8), b) < 1e-7
    L2 = L.clone()
    L2[0, 1, 0] += 1e-8
    assert 1e-10 < S.phi(H, L2) < 1e-7


def test_banded_error_equals_the_dense_one():
    n = 41
    L, ld = S.band_factor(n, seed=3)
    assert torch.equal(L, torch.tril(L)) and (L.diagonal() == 2).all()
    assert int(torch.count_nonzero(torch.tril(L, -S.BAND - 1))) == 0
    assert float(torch.tril(L, -1).abs().max()) <= 0.1
    b = torch.randn(n, 1, generator=torch.Generator().manual_seed(1), dtype=S.F64)
    x = torch.cholesky_solve(b, L)
    H = L @ L.T
    dense = S.eta(H[None], x[None], b[None])
    band = S.band_eta(ld, x, b)
    # H = L L^T rounded to fp64 for the dense one: they agree to that rounding
    assert band <= 4 * S.unit_roundoff(S.F64)
    assert abs(band - dense) <= 2 * S.unit_roundoff(S.F64)
    bad = S.band_eta(ld, x * (1 + 1e-9), b)
    assert 1e-10 < bad < 1e-8
    assert np.isfinite(bad)
