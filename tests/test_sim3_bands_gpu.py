"""GPU: every forward and backward op of Sim3 (lietorch group 4) through
lietorch_backends over the (theta, sigma) sweep of tests/sim3_bands.py, in f64
and f32, against tests/sim3_restatement.py (matrix exponential, left Jacobian
by autograd; held to account by test_sim3_restatement.py).  The sweep is the
full product of theta in {0, 1e-9, 1e-5, 1e-3, both sides of the logm switch
at 0.02 and of the w_coeffs switch at 0.05, 0.3, 1, 2, 3, pi - 1e-3, f64: pi -
1e-6, exp: beyond pi} with sigma in {0, 1e-9, -1e-5, 1e-3, 0.1, both sides of
+-0.5, 1, -2, 3}: all four (theta, sigma) combinations of w_coeffs, the
recurrence branch included, every branch of logm, quaternions of either sign
and unnormalised.  One more case runs 257 rows at (0.0499, 0.501), the
recurrence branch, across the 256-thread block edge.  test_sim3_host.py runs
the same rows through the same header on the host.

Error measure: |got - ref| / max(1, max |ref| of the row); group-valued
outputs as 4x4 matrices (either quaternion sign), and | |q| - 1 | apart.

f64 bounds: 4 x the largest error measured on an MI355X per (op, direction),
rounded up to one digit, never above the project's 1e-10 (table F64).
f32 bounds are derived, not measured: group 4 computes in fp64 and rounds once
on store, so a vector-valued output is within one f32 roundoff of the row's
scale, 2^-24; the bound is 2^-23.  A group-valued output is compared as a
matrix s R(q): the rounded quaternion enters R quadratically (2 roundoffs),
the rounded scale gives one and the renormalisation of the rounded quaternion
one more, so 8 * 2^-24 with | |q| - 1 | <= 2^-22.  What was measured stands
next to them (table F32_MEASURED).
"""
import pytest
import torch

import sim3_bands as B

pytestmark = pytest.mark.gpu

F64_CAP = 1e-10  # the project's bound for every fp64 Lie op
# f64, (op, direction): (largest error measured on an MI355X over sweep and
# block, asserted bound = 4 x measured rounded up to one digit).  matrix and
# projector came out equal to the reference bit for bit (it forms the same
# products); their bound is 4 roundoffs, 4 * 2^-52, in place of 4 x 0.  The
# host run of test_sim3_host.py gives the same figures to within a roundoff:
# the device's libm and compiler add nothing.
F64 = {
    ("exp", "fwd"): (4.42e-15, 2e-14),
    ("log", "fwd"): (2.01e-15, 9e-15),
    ("inv", "fwd"): (1.30e-15, 6e-15),
    ("mul", "fwd"): (9.48e-16, 4e-15),
    ("adj", "fwd"): (1.20e-15, 5e-15),
    ("adjT", "fwd"): (7.81e-16, 4e-15),
    ("act", "fwd"): (6.66e-16, 3e-15),
    ("act4", "fwd"): (8.65e-16, 4e-15),
    ("matrix", "fwd"): (0.00e+00, 9e-16),
    ("projector", "fwd"): (0.00e+00, 9e-16),
    ("Jinv", "fwd"): (5.59e-14, 3e-13),
    ("exp", "bwd"): (4.90e-14, 2e-13),
    ("log", "bwd"): (5.18e-14, 3e-13),
    ("inv", "bwd"): (1.31e-15, 6e-15),
    ("mul", "bwd"): (1.28e-14, 6e-14),
    ("adj", "bwd"): (1.30e-15, 6e-15),
    ("adjT", "bwd"): (1.66e-15, 7e-15),
    ("act", "bwd"): (8.01e-16, 4e-15),
    ("act4", "bwd"): (9.66e-16, 4e-15),
}
F64_QNORM = 1e-14  # a quaternion normalised in fp64: a few roundoffs

F32_VECTOR = 2.0 ** -23
F32_MATRIX = 8 * 2.0 ** -24
F32_QNORM = 2.0 ** -22
# f32, (op, direction): largest error measured on an MI355X (for the
# group-valued ops: matrix error, | |q| - 1 |)
F32_MEASURED = {
    ("exp", "fwd"): (8.71e-08, 3.7e-08),
    ("log", "fwd"): 5.81e-08,
    ("inv", "fwd"): (5.98e-08, 4.0e-08),
    ("mul", "fwd"): (9.15e-08, 3.8e-08),
    ("adj", "fwd"): 5.75e-08,
    ("adjT", "fwd"): 5.64e-08,
    ("act", "fwd"): 5.84e-08,
    ("act4", "fwd"): 5.88e-08,
    ("matrix", "fwd"): 5.64e-08,
    ("projector", "fwd"): 1.48e-08,
    ("Jinv", "fwd"): 5.67e-08,
    ("exp", "bwd"): 5.53e-08,
    ("log", "bwd"): 5.82e-08,
    ("inv", "bwd"): 5.69e-08,
    ("mul", "bwd"): 5.78e-08,
    ("adj", "bwd"): 5.71e-08,
    ("adjT", "bwd"): 5.87e-08,
    ("act", "bwd"): 5.78e-08,
    ("act4", "bwd"): 5.75e-08,
}

NAMES = {"exp": "expm", "log": "logm", "inv": "inv", "mul": "mul", "adj": "adj", "adjT": "adjT",
         "act": "act", "act4": "act4", "matrix": "as_matrix", "projector": "projector",
         "Jinv": "Jinv"}
DTYPES = {"f64": torch.float64, "f32": torch.float32}
GROUP = 4


@pytest.fixture(scope="module")
def lb(gpu):
    import dpvo_amd

    return dpvo_amd.load_extension("lietorch_backends")


def _bounds(op, direction, dt):
    """(bound of the row error, bound of | |q| - 1 |)."""
    if dt == "f64":
        b = F64[op, direction][1]
        assert b <= F64_CAP
        return b, F64_QNORM
    return (F32_MATRIX if direction == "fwd" and op in B.GROUP_VALUED else F32_VECTOR), F32_QNORM


@pytest.mark.parametrize("case", ["sweep", "block"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("op", B.FWD_OPS)
def test_forward_sweep(lb, gpu, op, dt, case):
    x, y, _, ref = B.case(op, False, dt, case)
    args = [t.to(gpu, DTYPES[dt]) for t in (x, y) if t is not None]
    out = getattr(lb, NAMES[op])(GROUP, *args)
    assert out.dtype == DTYPES[dt] and out.shape[0] == len(x)
    out = out.double().cpu().reshape(len(x), -1)
    err, qerr = B.forward_error(op, out, ref)
    print(f"SIM3 BANDS fwd op={op} {dt} {case} err={err:.3e} qnorm={qerr:.1e}")
    bound, qbound = _bounds(op, "fwd", dt)
    assert err <= bound
    assert qerr <= qbound


@pytest.mark.parametrize("case", ["sweep", "block"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("op", B.BWD_OPS)
def test_backward_sweep(lb, gpu, op, dt, case):
    x, y, g, refs = B.case(op, True, dt, case)
    args = [t.to(gpu, DTYPES[dt]) for t in (g, x, y) if t is not None]
    outs = getattr(lb, NAMES[op] + "_backward")(GROUP, *args)
    assert all(o.dtype == DTYPES[dt] for o in outs)
    err = B.backward_error([o.double().cpu() for o in outs], refs)
    print(f"SIM3 BANDS bwd op={op} {dt} {case} err={err:.3e}")
    assert err <= _bounds(op, "bwd", dt)[0]


# ---- the extension refuses operands the group-4 kernels would index out of bounds ----
F64T, F32T = torch.float64, torch.float32
BAD = [
    # (what, function, argument shapes / dtypes)
    ("7-wide data", "logm", [((5, 7), F64T)]),
    ("7-wide data with a point", "act", [((5, 7), F64T), ((5, 3), F64T)]),
    ("6-wide tangent", "expm", [((5, 6), F64T)]),
    ("6-wide tangent as Y", "adj", [((5, 8), F64T), ((5, 6), F64T)]),
    ("6-wide tangent as grad", "logm_backward", [((5, 6), F64T), ((5, 8), F64T)]),
    ("se3 data given to mul", "mul", [((5, 8), F64T), ((5, 7), F64T)]),
    ("7-wide grad of a group element", "inv_backward", [((5, 7), F64T), ((5, 8), F64T)]),
    ("fewer rows in Y", "mul", [((5, 8), F64T), ((4, 8), F64T)]),
    ("fewer rows in Y of Jinv", "Jinv", [((5, 8), F64T), ((4, 7), F64T)]),
    ("fewer rows in grad", "expm_backward", [((4, 8), F64T), ((5, 7), F64T)]),
    ("fewer rows in grad of act", "act_backward", [((4, 3), F64T), ((5, 8), F64T), ((5, 3), F64T)]),
    ("f32 Y with f64 X", "act4", [((5, 8), F64T), ((5, 4), F32T)]),
    ("f32 grad with f64 X", "expm_backward", [((5, 8), F32T), ((5, 7), F64T)]),
    ("f64 grad with f32 X", "adjT_backward", [((5, 7), F64T), ((5, 8), F32T), ((5, 7), F32T)]),
    ("1-D X", "logm", [((8,), F64T)]),
    ("1-D Y", "adjT", [((1, 8), F64T), ((7,), F64T)]),
    ("1-D grad", "logm_backward", [((7,), F64T), ((1, 8), F64T)]),
    ("3-D X", "projector", [((2, 3, 8), F64T)]),
    ("3-D Y", "act", [((6, 8), F64T), ((2, 3, 3), F64T)]),
    ("half precision", "expm", [((5, 7), torch.float16)]),
    ("half precision data", "Jinv", [((5, 8), torch.float16), ((5, 7), torch.float16)]),
]


@pytest.mark.parametrize("what,fn,specs", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_bad_operands_are_refused_before_launch(lb, gpu, what, fn, specs):
    args = [torch.ones(shape, dtype=dtype, device=gpu) for shape, dtype in specs]
    # the refusal is an argument check's own message (a status returned by the
    # launcher reads "... failed: ..."), and the operands are left untouched
    with pytest.raises(RuntimeError, match="lietorch_backends: ") as exc:
        getattr(lb, fn)(GROUP, *args)
    assert "failed" not in str(exc.value), what
    torch.cuda.synchronize(gpu)
    for a in args:
        assert bool((a == 1).all())
