"""CPU: the mask-injecting restatement (tests/update_grad_ref.py) that the
backward of the update operator is measured against: it equals update_ref with
default masks, its gradient matches a central finite difference, and in every
case of the GPU test the share of ReLU positions that an fp32 forward may
legitimately flip stays under the cap."""
import numpy as np
import pytest
import torch

import update_grad_ref as ugr
import update_ref


def setup(E, K0, kind, seed):
    c = ugr.make_case("cpu", E, K0, kind, seed)
    P = update_ref.to_torch(update_ref.formula_params(K0))
    return c, P


def run64(P, c, masks=None, pre=None):
    return ugr.update_masked(P, c["net"].double(), c["inp"].double(), c["corr"].double(), c["ix"],
                             c["jx"], c["gk"], c["gij"], masks=masks, pre=pre)


@pytest.mark.parametrize("case", [(17, 49, "dpvo", 0), (40, 49, "dup", 3), (33, 49, "fan_in", 2)],
                         ids=ugr.case_id)
def test_default_masks_equal_update_ref(case):
    c, P = setup(*case)
    pre = {}
    got = run64(P, c, pre=pre)
    want = update_ref.update_ref(P, c["net"].double(), c["inp"].double(), c["corr"].double(),
                                 c["ix"], c["jx"], c["gk"], c["gij"])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert tuple(pre) == ugr.RELUS
    # the masks it would read back reproduce it, and a flipped entry does not
    masks = {k: p > 0 for k, p in pre.items()}
    for a, b in zip(run64(P, c, masks=masks), want):
        assert torch.equal(a, b)
    masks["c1.0"] = ~masks["c1.0"]
    assert not torch.equal(run64(P, c, masks=masks)[0], want[0])


def test_gradient_matches_a_central_difference():
    E, K0 = 15, 49
    c, P = setup(E, K0, "dpvo", 0)
    cot = ugr.cotangents(E, 0, "cpu")
    pre = {}
    run64(P, c, pre=pre)
    masks = {k: p > 0 for k, p in pre.items()}  # frozen: the difference must not cross a kink
    g = ugr.grads(P, c, cot, masks=masks)
    names = ugr.names(K0)

    def loss(P2, c2):
        return float(sum((o * t).sum() for o, t in zip(run64(P2, c2, masks=masks), cot)))

    h = 1e-6
    spots = [("net", (3, 100)), ("corr", (7, 20)), ("agg_kk.g.weight", (5, 9))]
    for name, idx in spots:
        vals = []
        for sgn in (1.0, -1.0):
            P2 = {k: v.clone() for k, v in P.items()}
            c2 = {k: (v.double().clone() if k in ("net", "inp", "corr") else v) for k, v in c.items()}
            (c2 if name in c2 else P2)[name][idx] += sgn * h
            vals.append(loss(P2, c2))
        fd = (vals[0] - vals[1]) / (2 * h)
        an = float((g[("net", "inp", "corr").index(name)] if name in c else
                    g[3 + names.index(name)])[idx])
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (name, fd, an)


@pytest.mark.parametrize("case", ugr.CASES, ids=ugr.case_id)
def test_near_tie_share_is_under_the_cap(case):
    c, P = setup(*case)
    pre = {}
    with torch.no_grad():
        run64(P, c, pre=pre)
    share = ugr.near_tie_share(pre)
    print(f"NEARTIE {ugr.case_id(case)} share {share:.3e} (cap {ugr.NEAR_TIE_CAP:.0e})")
    assert share <= ugr.NEAR_TIE_CAP


def test_fan_in_scatters_four_edges_into_a_row_and_all_into_row_zero():
    c = ugr.make_case("cpu", 200, 49, "fan_in", 5)
    assert torch.equal(c["ix"], torch.arange(200) // 4) and not c["jx"].any()
