"""CPU: the fp64 restatement of the update operator (tests/update_ref.py)
reproduces the fixture that scripts/make_update_golden.py recorded from the
reference's own Update.forward (fork variant: neighbors_tensor indices, groups
kk and ii)."""
import numpy as np
import pytest
import torch

from conftest import golden
import update_ref


@pytest.fixture(scope="module")
def case():
    g = golden("update_fork_a")
    P = update_ref.to_torch(update_ref.formula_params(g["corr"].shape[1]))
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    i = lambda a: torch.as_tensor(np.asarray(a))
    out = update_ref.update_ref(P, t(g["net"]), t(g["inp"]), t(g["corr"]), i(g["ix"]), i(g["jx"]),
                                i(g["kk"]), i(g["ii"]), return_logits=True)
    return g, out


def test_fixture_is_fork_shaped(case):
    g, _ = case
    E = len(g["kk"])
    assert E == 48 and g["corr"].shape == (E, 882)
    assert g["ix"].min() >= 0 and g["ix"].max() < E and g["jx"].min() >= 0 and g["jx"].max() < E
    for k in ("net", "inp", "corr"):
        assert g[k].dtype == np.float32
    # more than one kk group with several members, and more than one ii group
    assert 1 < len(np.unique(g["kk"])) < E and len(np.unique(g["ii"])) > 1


def test_restatement_reproduces_reference(case):
    g, (net_out, d, w, logit) = case
    assert logit < 50.0  # the fork's clamp is inert on this fixture
    assert np.abs(net_out.numpy() - g["net_out"]).max() <= 1e-12
    # the fork adds ii * 1e-10 to d and w (net.py:331-337); the restatement does not
    assert np.abs(d.numpy() - g["d"]).max() <= 1e-9
    assert np.abs(w.numpy() - g["w"]).max() <= 1e-9


def test_formula_params_are_deterministic_and_scaled():
    a, b = update_ref.formula_params(49), update_ref.formula_params(49)
    assert list(a) == [n for n, _ in update_ref.param_shapes(49)] and len(a) == 50
    for k in a:
        assert np.array_equal(a[k], b[k])
    W = a["c1.0.weight"].astype(np.float64)
    assert abs(W.std() * np.sqrt(384) - 1.0) < 0.05 and abs(W.mean()) < 0.01
    assert np.abs(a["norm.weight"] - 1.0).max() > 0.2 and np.abs(a["norm.bias"]).max() > 0.1


def test_f16_operand_mode_only_rounds_linear_operands():
    E, K0 = 20, 49
    P = update_ref.to_torch(update_ref.formula_params(K0))
    ii, jj, kk = update_ref.dpvo_graph(E, M=4, seed=1)
    net, inp, corr = (torch.as_tensor(a, dtype=torch.float64) for a in update_ref.inputs(E, K0, 1))
    ix, jx = (torch.as_tensor(a) for a in update_ref.neighbors_ref(kk, jj))
    args = (net, inp, corr, ix, jx, torch.as_tensor(kk), torch.as_tensor(ii * 12345 + jj))
    ref = update_ref.update_ref(P, *args)
    emu = update_ref.update_ref(P, *args, f16_operand=True)
    rel = float((emu[0] - ref[0]).abs().max() / ref[0].abs().max())
    assert 1e-6 < rel < 5e-3, rel  # fp16 operand rounding (2^-11 per operand), not fp64 noise
