"""GPU: spd_solve.hip through cuda_ba.spd_solve / spd_solve_factored at every
residency of its working matrix (LDS, LDS above 64 KB, HBM), on both sides of
each boundary, past one trip of its 256-wide loops, at n = 1 and 2, on
ill-conditioned systems, and on every failure path; see spd_cases for the
error measures, the reference and the bars.  Each test prints its ratios
(error over bar); DESIGN.md's spd_solve section quotes the largest."""
import json
import os
import subprocess
import sys

import pytest
import torch

import spd_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    from dpvo_amd.ba import _cuda_ba

    return _cuda_ba


def solve(ba, H, b, dev):
    x, L, info = ba.spd_solve(H.to(dev), b.to(dev))
    return x.cpu(), L.cpu(), info.cpu()


def strict_upper_is_zero(L):
    return int(torch.count_nonzero(torch.triu(L, diagonal=1))) == 0


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("case", S.ACCURACY, ids=S.case_id)
def test_backward_errors(gpu, ba, case):
    dt, n, k, cond, res = case
    assert S.residency(n, k, dt) == res
    ref = S.reference(case)
    H, b = ref["H"], ref["b"]
    x, L, info = solve(ba, H, b, gpu)
    assert info.tolist() == [0]
    assert x.dtype == L.dtype == dt and x.shape == b.shape and L.shape == H.shape
    assert strict_upper_is_zero(L)
    x2 = ba.spd_solve_factored(L.to(gpu), b.to(gpu)).cpu()
    eta_bar, phi_bar = bars = S.bars(ref)
    got = {"eta": S.eta(H, x, b), "eta_factored": S.eta(H, x2, b), "phi": S.phi(H, L)}
    ratio = {"eta": got["eta"] / eta_bar, "eta_factored": got["eta_factored"] / eta_bar,
             "phi": got["phi"] / phi_bar}
    print(f"\n[spd] {S.case_id(case)} {res} " + " ".join(f"{t}={got[t]:.2e} ratio={ratio[t]:.3f}" for t in got)
          + f" ref eta={ref['eta']:.2e} phi={ref['phi']:.2e} bars={bars[0]:.2e}/{bars[1]:.2e}")
    assert all(v <= 1.0 for v in ratio.values()), (got, bars)


# ------------------------------------------------------------------ only the lower triangle is read
@pytest.mark.parametrize("n", [40, 150])
def test_upper_triangle_is_never_read(gpu, ba, n):
    assert S.residency(n, 1, S.F64) == (S.LDS if n == 40 else S.HBM)
    H, b = S.spd(n, 1, 10.0, S.F64, seed=n)
    nan_above = torch.triu(torch.full_like(H, float("nan")), diagonal=1)
    x, L, info = solve(ba, H, b, gpu)
    xn, Ln, infon = solve(ba, torch.tril(H) + nan_above, b, gpu)
    assert info.tolist() == infon.tolist() == [0]
    assert torch.equal(x, xn) and torch.equal(L, Ln) and torch.isfinite(x).all()
    y = ba.spd_solve_factored(L.to(gpu), b.to(gpu)).cpu()
    yn = ba.spd_solve_factored((L + nan_above).to(gpu), b.to(gpu)).cpu()
    assert torch.equal(y, yn) and torch.isfinite(y).all()


# ------------------------------------------------------------------ determinism, item independence
@pytest.mark.parametrize("dtype,n,res", [(S.F64, 40, S.LDS), (S.F64, 120, S.RAISED), (S.F64, 150, S.HBM),
                                         (S.F32, 258, S.HBM)])
def test_six_copies_one_answer(gpu, ba, dtype, n, res):
    assert S.residency(n, 1, dtype) == res
    H, b = S.spd(n, 1, 10.0, dtype, seed=n)
    x1, L1, i1 = solve(ba, H, b, gpu)
    x6, L6, i6 = solve(ba, H.repeat(6, 1, 1), b.repeat(6, 1, 1), gpu)
    xa, La, ia = solve(ba, H, b, gpu)
    assert i1.tolist() == ia.tolist() == [0] and i6.tolist() == [0] * 6
    assert torch.equal(x1, xa) and torch.equal(L1, La)
    for i in range(6):
        assert torch.equal(x6[i], x1[0]) and torch.equal(L6[i], L1[0]), i


def test_factor_does_not_depend_on_residency(gpu, ba):
    """The header's "same code, global addresses": k = 1 factors in LDS with
    the mirrored upper triangle, k = 400 in the HBM working copy."""
    assert S.residency(100, 1, S.F32) == S.LDS and S.residency(100, 400, S.F32) == S.HBM
    H, b = S.spd(100, 400, 10.0, S.F32, seed=5)
    _, L_lds, i0 = solve(ba, H, b[..., :1].contiguous(), gpu)
    _, L_hbm, i1 = solve(ba, H, b, gpu)
    assert i0.tolist() == i1.tolist() == [0]
    assert torch.equal(L_lds, L_hbm)


# ------------------------------------------------------------------ failures
@pytest.mark.parametrize("kinds", [("col0", "last"), ("nan_pivot", "nan_offdiag")], ids="-".join)
@pytest.mark.parametrize("dtype,n,res", [(S.F64, 40, S.LDS), (S.F64, 150, S.HBM), (S.F32, 210, S.HBM)])
def test_failures_next_to_healthy_items(gpu, ba, dtype, n, res, kinds):
    assert S.residency(n, 1, dtype) == res
    H, b = S.spd(n, 1, 10.0, dtype, seed=n, batch=5)
    Hb = H.clone()
    want = [0] * 5
    poisoned = {}
    for item, kind in zip((1, 3), kinds):
        Hb[item], want[item], poisoned[item] = S.break_at(H[item], kind)
    assert want[1] != want[3]
    x, L, info = solve(ba, Hb, b, gpu)
    assert info.tolist() == want
    x0, L0, info0 = solve(ba, H, b, gpu)  # the unbroken matrices
    assert info0.tolist() == [0] * 5
    assert strict_upper_is_zero(L)
    for item in (0, 2, 4):
        xa, La, ia = solve(ba, H[item:item + 1], b[item:item + 1], gpu)
        assert ia.tolist() == [0]
        assert torch.equal(x[item], xa[0]) and torch.equal(L[item], La[0]), item
        assert torch.equal(x[item], x0[item]) and torch.equal(L[item], L0[item]), item
    for item in (1, 3):
        c = want[item] - 1  # the failed column
        assert int(torch.count_nonzero(x[item])) == 0
        before, before0 = L[item][:, :c].clone(), L0[item][:, :c].clone()
        if poisoned[item] is not None:
            # a NaN below the diagonal at (i, j) is l_ij, and reaches row i of every later
            # column through a_ic -= l_ij l_cj; every other entry before column i is untouched
            i, j = poisoned[item]
            assert i == c and torch.isnan(before[i, j:]).all()
            before[i, j:] = 0
            before0[i, j:] = 0
        assert torch.equal(before, before0), item


# ------------------------------------------------------------------ solve-only leaves its factor alone
@pytest.mark.parametrize("n", [66, 150])
def test_solve_only_does_not_write_its_factor(gpu, ba, n):
    assert S.residency(n, 1, S.F64) == (S.LDS if n == 66 else S.HBM)
    H, b = S.spd(n, 1, 10.0, S.F64, seed=n)
    L = ba.spd_solve(H.to(gpu), b.to(gpu))[1]
    kept = L.clone()
    x = ba.spd_solve_factored(L, b.to(gpu))
    assert torch.equal(L, kept)
    eta_ref = S.eta(H, S.reference_solve(H, b)[0], b)
    assert S.eta(H, x, b) <= S.ETA_MARGIN * max(eta_ref, S.unit_roundoff(S.F64))  # a solve happened


# ------------------------------------------------------------------ binding
def test_leading_dims_are_a_batch(gpu, ba):
    n = 12
    H, b = S.spd(n, 2, 10.0, S.F64, seed=9, batch=6)
    x, L, info = solve(ba, H.view(2, 3, n, n), b.view(2, 3, n, 2), gpu)
    assert x.shape == (2, 3, n, 2) and L.shape == (2, 3, n, n) and info.shape == (2, 3)
    for i in range(6):
        xa, La, ia = solve(ba, H[i:i + 1], b[i:i + 1], gpu)
        assert torch.equal(x.view(6, n, 2)[i], xa[0]) and torch.equal(L.view(6, n, n)[i], La[0])
        assert int(info.view(6)[i]) == int(ia) == 0


def test_non_contiguous_inputs(gpu, ba):
    n = 20
    H, b = S.spd(n, 3, 10.0, S.F32, seed=11, batch=2)
    H, b = H.to(gpu), b.to(gpu)
    Hn = H.transpose(-1, -2).contiguous().transpose(-1, -2)
    bn = b.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not Hn.is_contiguous() and not bn.is_contiguous()
    assert torch.equal(Hn, H) and torch.equal(bn, b)
    x, L, info = ba.spd_solve(H, b)
    xn, Ln, infon = ba.spd_solve(Hn, bn)
    assert torch.equal(x, xn) and torch.equal(L, Ln) and torch.equal(info, infon)
    Ln2 = L.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert torch.equal(ba.spd_solve_factored(L, b), ba.spd_solve_factored(Ln2, bn))


# ------------------------------------------------------------------ the largest launch
def test_largest_size_the_layer_admits(gpu):
    """Solve-only at n = 8184 = 6 x 1364 free poses (fp64, k = 1, the factor
    read in HBM, the column scratch at the LDS limit), in a process of its own
    under a 60 s limit.  O(n^2); no factorisation at this size (O(n^3) on one
    workgroup)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "spd_cases.py")], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    u = S.unit_roundoff(S.F64)
    bar = S.ETA_MARGIN * max(out["eta_ref"], u)
    print(f"\n[spd] largest launch n={out['n']} eta={out['eta_gpu']:.2e} ref={out['eta_ref']:.2e} "
          f"ratio={out['eta_gpu'] / bar:.3f} device call {out['seconds']:.3f} s")
    assert out["n"] == S.MAX_N_F64 and out["factor_unchanged"]
    assert out["eta_gpu"] <= bar, out


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize("n,res", [(96, S.RAISED), (150, S.HBM)])
def test_cholesky_solver_gradients(gpu, n, res):
    """CholeskySolver against autograd through torch.linalg.solve; at n = 150
    the backward's solve reads the stored factor in HBM."""
    from dpvo_amd.ba import CholeskySolver

    assert S.residency(n, 2, S.F64) == res
    H, b = S.spd(n, 2, 10.0, S.F64, seed=n)
    c = torch.randn(b.shape, generator=torch.Generator().manual_seed(2), dtype=S.F64).to(gpu)
    grads = []
    for f in (CholeskySolver.apply, torch.linalg.solve):
        h, v = H.to(gpu).requires_grad_(), b.to(gpu).requires_grad_()
        x = f(0.5 * (h + h.transpose(-1, -2)), v)
        (c * x).sum().backward()
        grads.append((x.detach(), h.grad, v.grad))
    for got, ref in zip(*grads):
        torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-10)
    assert grads[0][1].abs().max() > 0
