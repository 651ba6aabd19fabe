"""GPU: every forward and backward op of SO3 / SE3 (lietorch groups 1 and 3)
through lietorch_backends over the angle sweep of tests/lie_bands.py, in f64
and f32, against tests/se3_restatement.py (matrix exponential + autograd,
itself held to 1e-13 by test_se3_restatement.py).  The sweep walks theta
through 0, both sides of the old 1e-6 switch, the band up to 5e-2 where the
closed-form coefficients cancel, pi - 1e-3 (f64: pi - 1e-6) and, for exp,
beyond pi; quaternions come with either sign and unnormalised.  One more case
runs 257 rows at theta = 1e-4 across the 256-thread block edge.  SE3 is also
compared with Sim3 (group 4) on the lifted element, and the argument checks
of the extension are exercised (nothing may reach a kernel with bad sizes).

Error measure: |got - ref| / max(1, max |ref| of the row); group-valued
outputs as matrices (either quaternion sign) and of unit norm; log within
1e-3 of pi by the round trip Exp_ref(log(X)) == X.
"""
import functools

import pytest
import torch

import lie_bands as B

pytestmark = pytest.mark.gpu

F64_BOUND = 1e-10  # every case, bands included

# f32: largest error of the sweep on an MI355X per (group, op, direction), and
# the asserted bound = 4 x measured rounded up to one digit (other seeds and
# libm differences, no more).  No bound may exceed F32_CAP: 2e-5 is about 300
# f32 roundoffs at unit scale, more than that means cancellation.
F32_CAP = 2e-5
F32 = {  # (group, op, direction): (measured, asserted bound)
    (1, "exp", "fwd"): (1.45e-07, 6e-7),
    (1, "log", "fwd"): (1.13e-07, 5e-7),
    (1, "inv", "fwd"): (7.03e-08, 3e-7),
    (1, "mul", "fwd"): (1.82e-07, 8e-7),
    (1, "adj", "fwd"): (2.91e-07, 2e-6),
    (1, "adjT", "fwd"): (2.22e-07, 9e-7),
    (1, "act", "fwd"): (2.02e-07, 9e-7),
    (1, "act4", "fwd"): (3.67e-07, 2e-6),
    (1, "matrix", "fwd"): (3.38e-07, 2e-6),
    (1, "projector", "fwd"): (4.10e-08, 2e-7),
    (1, "Jinv", "fwd"): (1.36e-07, 6e-7),
    (1, "exp", "bwd"): (1.87e-07, 8e-7),
    (1, "log", "bwd"): (1.90e-07, 8e-7),
    (1, "inv", "bwd"): (2.73e-07, 2e-6),
    (1, "mul", "bwd"): (2.89e-07, 2e-6),
    (1, "adj", "bwd"): (3.75e-07, 2e-6),
    (1, "adjT", "bwd"): (3.05e-07, 2e-6),
    (1, "act", "bwd"): (2.99e-07, 2e-6),
    (1, "act4", "bwd"): (4.36e-07, 2e-6),
    (3, "exp", "fwd"): (1.45e-07, 6e-7),
    (3, "log", "fwd"): (1.39e-07, 6e-7),
    (3, "inv", "fwd"): (1.87e-07, 8e-7),
    (3, "mul", "fwd"): (2.29e-07, 1e-6),
    (3, "adj", "fwd"): (4.13e-07, 2e-6),
    (3, "adjT", "fwd"): (3.19e-07, 2e-6),
    (3, "act", "fwd"): (3.05e-07, 2e-6),
    (3, "act4", "fwd"): (4.20e-07, 2e-6),
    (3, "matrix", "fwd"): (3.38e-07, 2e-6),
    (3, "projector", "fwd"): (3.98e-08, 2e-7),
    (3, "Jinv", "fwd"): (2.08e-07, 9e-7),
    (3, "exp", "bwd"): (3.42e-07, 2e-6),
    (3, "log", "bwd"): (1.54e-07, 7e-7),
    (3, "inv", "bwd"): (3.44e-07, 2e-6),
    (3, "mul", "bwd"): (3.93e-07, 2e-6),
    (3, "adj", "bwd"): (7.04e-07, 3e-6),
    (3, "adjT", "bwd"): (5.50e-07, 3e-6),
    (3, "act", "bwd"): (3.65e-07, 2e-6),
    (3, "act4", "bwd"): (3.32e-07, 2e-6),
}

NAMES = {"exp": "expm", "log": "logm", "inv": "inv", "mul": "mul", "adj": "adj", "adjT": "adjT",
         "act": "act", "act4": "act4", "matrix": "as_matrix", "projector": "projector",
         "Jinv": "Jinv"}
DTYPES = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(scope="module")
def lb(gpu):
    import dpvo_amd

    return dpvo_amd.load_extension("lietorch_backends")


@functools.lru_cache(maxsize=None)
def _case(group, op, backward, dt, case):
    """Inputs rounded to the kernel's dtype (as fp64) and the reference at them."""
    theta, x, y, g = B.inputs(group, op, backward, dt == "f64", case)
    r = lambda t: None if t is None else t.to(DTYPES[dt]).double()  # noqa: E731
    x, y, g = r(x), r(y), r(g)
    ref = B.reference_bwd(group, op, g, x, y) if backward else B.reference_fwd(group, op, x, y)
    return theta, x, y, g, ref


def _bound(group, op, direction, dt):
    if dt == "f64":
        return F64_BOUND
    b = F32[group, op, direction][1]
    assert b <= F32_CAP
    return b


@pytest.mark.parametrize("case", ["sweep", "block"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("op", B.FWD_OPS)
@pytest.mark.parametrize("group", [1, 3])
def test_forward_sweep(lb, gpu, group, op, dt, case):
    theta, x, y, _, ref = _case(group, op, False, dt, case)
    args = [t.to(gpu, DTYPES[dt]) for t in (x, y) if t is not None]
    out = getattr(lb, NAMES[op])(group, *args)
    assert out.dtype == DTYPES[dt] and out.shape[0] == len(x)
    out = out.double().cpu().reshape(len(x), -1)
    err = B.forward_error(group, op, theta, x, out, ref)
    print(f"BANDS fwd group={group} op={op} {dt} {case} err={err:.3e}")
    assert err <= _bound(group, op, "fwd", dt)


@pytest.mark.parametrize("case", ["sweep", "block"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("op", B.BWD_OPS)
@pytest.mark.parametrize("group", [1, 3])
def test_backward_sweep(lb, gpu, group, op, dt, case):
    theta, x, y, g, refs = _case(group, op, True, dt, case)
    args = [t.to(gpu, DTYPES[dt]) for t in (g, x, y) if t is not None]
    outs = getattr(lb, NAMES[op] + "_backward")(group, *args)
    assert len(outs) == len(refs)
    assert all(o.dtype == DTYPES[dt] for o in outs)
    err = max(B.row_error(o.double().cpu(), r) for o, r in zip(outs, refs))
    print(f"BANDS bwd group={group} op={op} {dt} {case} err={err:.3e}")
    assert err <= _bound(group, op, "bwd", dt)


@pytest.mark.parametrize("op", ["exp", "log", "inv", "mul", "act", "adj", "Jinv"])
def test_se3_agrees_with_lifted_sim3(lb, gpu, op):
    """Group 3 against group 4 at s = 1, sigma = 0 (f64): the two share no
    coefficient code (lie.hip's closed forms / series, sim3.hpp's W series and
    dual numbers), so agreement to 1e-10 over the sweep pins both."""
    theta, x, y, _ = B.inputs(3, op, False, True, "sweep")
    n = len(x)
    zero, one = torch.zeros(n, 1, dtype=torch.float64), torch.ones(n, 1, dtype=torch.float64)
    lift_t = lambda a: torch.cat([a, zero], 1)  # noqa: E731
    lift_g = lambda d: torch.cat([d, one], 1)  # noqa: E731
    x4 = lift_t(x) if op == "exp" else lift_g(x)
    y4 = None if y is None else lift_g(y) if op == "mul" else lift_t(y) if op in ("adj", "Jinv") else y
    a3 = [t.to(gpu) for t in (x, y) if t is not None]
    a4 = [t.to(gpu) for t in (x4, y4) if t is not None]
    o3 = getattr(lb, NAMES[op])(3, *a3).cpu()
    o4 = getattr(lb, NAMES[op])(4, *a4).cpu()
    if op in B.GROUP_VALUED:
        assert float((o4[:, 7] - 1).abs().max()) <= F64_BOUND
        err = B.row_error(B.as_matrix(3, o4[:, :7]), B.as_matrix(3, o3))
    elif op in ("log", "adj", "Jinv"):
        assert float(o4[:, 6].abs().max()) <= F64_BOUND  # no sigma
        err = B.row_error(o4[:, :6], o3)
    else:
        err = B.row_error(o4, o3)
    print(f"BANDS se3-vs-sim3 op={op} err={err:.3e}")
    assert err <= F64_BOUND


# ---- the extension refuses operands the kernels would index out of bounds ----
BAD = [
    # (what, function, group, argument shapes / dtypes)
    ("wrong last dim of X", "logm", 3, [((5, 6), torch.float64)]),
    ("wrong last dim of the tangent", "expm", 3, [((5, 7), torch.float64)]),
    ("wrong last dim of Y", "act", 3, [((5, 7), torch.float64), ((5, 4), torch.float64)]),
    ("wrong last dim of grad", "logm_backward", 3, [((5, 7), torch.float64), ((5, 7), torch.float64)]),
    ("so3 data given to se3", "inv", 3, [((5, 4), torch.float64)]),
    ("fewer rows in Y", "mul", 3, [((5, 7), torch.float64), ((4, 7), torch.float64)]),
    ("fewer rows in grad", "expm_backward", 1, [((4, 4), torch.float64), ((5, 3), torch.float64)]),
    ("more rows in X than grad, Y", "adj_backward", 3,
     [((4, 6), torch.float64), ((5, 7), torch.float64), ((4, 6), torch.float64)]),
    ("f32 grad with f64 X", "expm_backward", 3, [((5, 7), torch.float32), ((5, 6), torch.float64)]),
    ("f32 Y with f64 X", "adj", 1, [((5, 4), torch.float64), ((5, 3), torch.float32)]),
    ("f64 grad with f32 X", "act_backward", 3,
     [((5, 3), torch.float64), ((5, 7), torch.float32), ((5, 3), torch.float32)]),
    ("1-D X", "logm", 3, [((7,), torch.float64)]),
    ("1-D Y", "act", 1, [((1, 4), torch.float64), ((3,), torch.float64)]),
    ("1-D grad", "inv_backward", 3, [((7,), torch.float64), ((1, 7), torch.float64)]),
    ("3-D X", "as_matrix", 3, [((2, 3, 7), torch.float64)]),
    ("half precision", "expm", 3, [((5, 6), torch.float16)]),
]


@pytest.mark.parametrize("what,fn,group,specs", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_bad_operands_are_refused_before_launch(lb, gpu, what, fn, group, specs):
    args = [torch.ones(shape, dtype=dtype, device=gpu) for shape, dtype in specs]
    # the refusal is an argument check's own message (a status returned by the
    # launcher reads "... failed: ..."), and the device is left untouched
    with pytest.raises(RuntimeError, match="lietorch_backends: ") as exc:
        getattr(lb, fn)(group, *args)
    assert "failed" not in str(exc.value), what
    torch.cuda.synchronize(gpu)
    for a in args:
        assert bool((a == 1).all())


def test_cpu_operand_is_refused(lb, gpu):
    with pytest.raises(RuntimeError):
        lb.logm(3, torch.ones(5, 7, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        lb.mul(3, torch.ones(5, 7, dtype=torch.float64, device=gpu),
               torch.ones(5, 7, dtype=torch.float64))
