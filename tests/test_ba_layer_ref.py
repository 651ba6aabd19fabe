"""CPU: the restatement the GPU BA-layer tests compare against (ba_layer_ref)
is itself pinned: to oracle/cpu_baseline.ba_step, to the reference's recorded
fp64 outputs, to its own finite differences, and every case to the margins
and contents the GPU tests rely on."""
import numpy as np
import pytest
import torch
from conftest import golden

import ba_layer_ref as R
import cpu_baseline


def _ba_step(c):
    return cpu_baseline.ba_step(c.poses, c.patches, c.intr[0], c.targets, c.weights, c.lmbda, c.ii,
                                c.jj, c.kk, c.fixedp, ep=c.ep, bounds=c.bounds)


@pytest.mark.parametrize("name", ["b", "c_63", "c_64", "c_65", "c_257", "d_ba_py_a", "d_ba_py_b", "e"])
def test_restatement_equals_ba_step(name):
    c = R.case(name)
    P, K, aux = c.run()
    Pr, Kr = _ba_step(c)
    assert not aux["failed"]
    assert (P - Pr).abs().max() < 1e-10, (P - Pr).abs().max()
    assert (K - Kr).abs().max() < 1e-10, (K - Kr).abs().max()


@pytest.mark.parametrize("fx", ["ba_py_a", "ba_py_b"])
def test_restatement_equals_recorded_reference(fx):
    z = golden(fx)
    P, K, _ = R.case("d_" + fx).run()
    np.testing.assert_allclose(P.numpy(), z["out_poses64"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(K.numpy(), z["out_patches64"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", ["a_p1", "a_p3", "b"])
def test_restatement_gradcheck(name):
    c = R.case(name)
    cot = R.cotangents(c)

    def f(P, K, T, W):
        p, k, _ = R.ba_layer(P, K, c.intr, T, W, c.lmbda, c.ii, c.jj, c.kk, c.bounds, c.ep, c.fixedp,
                             c.structure_only, c.n)
        return R.act(p, cot["pts"]), k

    args = [x.clone().requires_grad_() for x in (c.poses, c.patches, c.targets, c.weights)]
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("name", R.GPU_CASES)
def test_case_margins(name):
    c = R.case(name)
    gate_ok, clamp_ok = R.margins(c)
    assert gate_ok and clamp_ok
    _, _, aux = c.run()
    assert aux["failed"] == (name == "h")
    if name != "h":
        assert int(aux["open"].sum()) >= 1


def test_case_contents():
    e = R.gate_content(R.case("e"))
    assert e["ok"], e
    b = R.case("b")
    assert len(set(b.kk.tolist())) < b.patches.shape[0]           # a patch with no edge
    assert (b.ii == b.jj).any() and ((b.ii < b.fixedp) & (b.jj < b.fixedp)).any()
    pairs = list(zip(b.kk.tolist(), b.jj.tolist()))
    assert len(set(pairs)) < len(pairs) and b.kk.tolist() != sorted(b.kk.tolist())
    g = R.case("g")
    assert 6 * (g.n - g.fixedp) == 138 and g.ii.numel() == 600
    db = R.case("d_ba_py_b").run()[2]
    assert int((~db["open"]).sum()) == 2                          # two edges outside the bounds
    for fx in ("d_ba_py_a", "d_ba_py_b"):
        a = R.case(fx).run()[2]
        assert a["Z"].min() > 0.7 and a["rnorm"].max() < 0.4


@pytest.mark.parametrize("name", ["b", "c_65"])
def test_chained_cases_see_the_derivative_of_the_jacobians(name):
    """The two-call GPU test exists to catch a backward that treats Ji / Jj / Jz
    as constants: on its cases that gradient is off by far more than any bound."""
    c = R.case(name)
    cot = R.cotangents(c)
    full = R.ref_grads(c, cot, chain=2)
    const = R.ref_grads(c, cot, chain=2, constant_jacobians=True)
    for t in ("g_poses", "g_patches"):
        off = float((full[t] - const[t]).abs().max() / full[t].abs().max())
        assert off > 1e-4, (t, off)


def test_tangent_conversion():
    """to_tangent against the derivative of f(Exp(xi) T) at xi = 0."""
    g = torch.Generator().manual_seed(0)
    T = R.se3_exp(torch.randn(4, 6, generator=g, dtype=torch.float64))
    pts = torch.randn(4, 3, 3, generator=g, dtype=torch.float64)
    c = torch.randn(4, 3, 3, generator=g, dtype=torch.float64)
    Tl = T.clone().requires_grad_()
    (c * R.act(Tl, pts)).sum().backward()
    xi = torch.zeros(4, 6, dtype=torch.float64, requires_grad=True)
    (c * R.act(R.se3_mul(R.se3_exp(xi), T), pts)).sum().backward()
    assert (R.to_tangent(T, Tl.grad) - xi.grad).abs().max() < 1e-12
