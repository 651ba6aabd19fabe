"""CPU: the C oracle's SO3 / SE3 (oracle.lie_fwd / lie_bwd, the so3.h / se3.h
restatement of oracle/dpvo_oracle.c) over the whole fp64 angle sweep of
tests/lie_bands.py against tests/se3_restatement.py, at the project's 1e-10.
The oracle is what test_lie_gpu.py holds the kernels to, so it has to be right
where the closed-form coefficients cancel (theta from 1e-6 to 1e-2) and next
to pi as well."""
import pytest
import torch

import lie_bands as B
import oracle

BOUND = 1e-10


def _t(a):
    return torch.from_numpy(a).to(torch.float64)


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("op", B.FWD_OPS)
def test_oracle_forward_sweep(group, op):
    theta, x, y, _ = B.inputs(group, op, False, True, "sweep")
    xn, yn = B.to_numpy(x, y)
    out = _t(oracle.lie_fwd(group, op, xn, yn))
    err = B.forward_error(group, op, theta, x, out, B.reference_fwd(group, op, x, y))
    print(f"oracle fwd group={group} {op}: {err:.2e}")
    assert err <= BOUND


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("op", B.BWD_OPS)
def test_oracle_backward_sweep(group, op):
    theta, x, y, g = B.inputs(group, op, True, True, "sweep")
    gn, xn, yn = B.to_numpy(g, x, y)
    outs = oracle.lie_bwd(group, op, gn, xn, yn)
    refs = B.reference_bwd(group, op, g, x, y)
    assert len(outs) == len(refs)
    errs = [B.row_error(_t(o), r) for o, r in zip(outs, refs)]
    print(f"oracle bwd group={group} {op}: {errs}")
    assert max(errs) <= BOUND
