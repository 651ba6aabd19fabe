"""Sim3 (lietorch group 4) on the GPU against the fp64 torch restatement of
tests/sim3_restatement.py: the 11 forward ops through lietorch_backends, the
reference's property tests (dpvo/lietorch/run_tests.py) on the Sim3 class,
gradients through the class API against the restatement's autograd Jacobians
at 1e-8 (the derivative is exact here, so the bound is that of SO3 / SE3, not
the reference's 1e-3 for Sim3), projective_ops.transform with Sim3 poses, and
the C ABI.

The rows here are general ones plus theta, sigma in {0, 1e-9, 1e-5, 1e-3}.
The switches of sim3.hpp (theta = 0.02 and 0.05, |sigma| = 0.5), the
recurrence branch, |sigma| > 0.7, angles next to and beyond pi, w < 0, the
backward ops through lietorch_backends and f32 backward are swept by
test_sim3_bands_gpu.py (and test_sim3_host.py on the CPU)."""
import numpy as np
import pytest
import torch

import sim3_restatement as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
SMALL = [0.0, 1e-9, 1e-5, 1e-3]
FWD = [("exp", "expm"), ("log", "logm"), ("inv", "inv"), ("mul", "mul"), ("adj", "adj"),
       ("adjT", "adjT"), ("act", "act"), ("act4", "act4"), ("matrix", "as_matrix"),
       ("projector", "projector"), ("Jinv", "Jinv")]


@pytest.fixture(scope="module")
def lb(gpu):
    import dpvo_amd

    return dpvo_amd.load_extension("lietorch_backends")


@pytest.fixture(scope="module")
def Sim3(gpu):
    from dpvo_amd.lietorch import Sim3

    return Sim3


def _tangents(n, seed):
    """|phi| up to 2.5, sigma in +-0.7, tau ~ N(0, 1); the first rows hit the
    small-argument branches: (theta, sigma) in {0, 1e-9, 1e-5, 1e-3}^2 with a
    translation of order 1, then sigma = 0 exactly with a large theta."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, 7, dtype=F64, generator=g)
    axis = torch.randn(n, 3, dtype=F64, generator=g)
    axis = axis / axis.norm(dim=1, keepdim=True)
    a[:, 3:6] = axis * 2.5 * torch.rand(n, 1, dtype=F64, generator=g)
    a[:, 6] = 0.7 * (2 * torch.rand(n, dtype=F64, generator=g) - 1)
    k = 0
    for theta in SMALL:
        for sigma in SMALL:
            a[k, 3:6] = theta * axis[k]
            a[k, 6] = sigma
            k += 1
    a[k, 3:6] = 2.2 * axis[k]
    a[k, 6] = 0.0
    return a


def _elements(n, seed):
    """Sim3 data built directly from (t, axis-angle, sigma) of _tangents, with
    the quaternion scaled by 1.3 (normalised on load)."""
    a = _tangents(n, seed)
    theta = a[:, 3:6].norm(dim=1, keepdim=True)
    axis = torch.where(theta > 0, a[:, 3:6] / theta.clamp(min=1e-300), torch.zeros_like(a[:, 3:6]))
    q = torch.cat([torch.sin(theta / 2) * axis, torch.cos(theta / 2)], 1)
    return torch.cat([a[:, :3], 1.3 * q, torch.exp(a[:, 6:7])], 1)


def _reference(op, x, y):
    """What each op must return, from the restatement; group elements as 4x4."""
    if op == "exp":
        return R.Exp(x)
    M = R.from_data(x)
    if op == "log":
        return R.Log(M)
    if op == "inv":
        return R.inv(M)
    if op == "mul":
        return M @ R.from_data(y)
    if op == "adj":
        return (R.Adj_matrix(M) @ y[..., None])[..., 0]
    if op == "adjT":
        return (R.Adj_matrix(M).transpose(1, 2) @ y[..., None])[..., 0]
    if op == "act":
        return (M[:, :3, :3] @ y[..., None])[..., 0] + M[:, :3, 3]
    if op == "act4":
        return (M @ y[..., None])[..., 0]
    if op == "matrix":
        return M
    if op == "projector":
        return R.projector(x)
    if op == "Jinv":
        return R.Jinv(M, y)
    raise KeyError(op)


@pytest.mark.parametrize("op,name", FWD)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_forward_matches_restatement(lb, gpu, op, name, dtype):
    n = 257  # not a multiple of the block
    x = _tangents(n, 0) if op == "exp" else _elements(n, 0)
    y = None
    if op == "mul":
        y = _elements(n, 1)[torch.randperm(n, generator=torch.Generator().manual_seed(2))]
    elif op in ("adj", "adjT", "Jinv"):
        y = torch.randn(n, 7, dtype=F64, generator=torch.Generator().manual_seed(3))
    elif op in ("act", "act4"):
        y = torch.randn(n, 3 if op == "act" else 4, dtype=F64,
                        generator=torch.Generator().manual_seed(4))
    args = [x.to(gpu, dtype)] + ([y.to(gpu, dtype)] if y is not None else [])
    out = getattr(lb, name)(4, *args).double().cpu()
    assert torch.isfinite(out).all()
    # the reference sees the kernel's own (rounded) inputs
    ref = _reference(op, *[a.double().cpu() for a in args], *([None] if y is None else []))
    if op in ("exp", "inv", "mul"):
        assert out.shape == (n, 8)
        out = R.from_data(out)
    tol = 1e-10 if dtype == torch.float64 else 2e-4
    np.testing.assert_allclose(out.reshape(n, -1).numpy(), ref.reshape(n, -1).numpy(),
                               rtol=tol, atol=tol)


# ---- the reference's property tests (run_tests.py:16-51), tolerance 1e-8 ----
def test_exp_log(Sim3, gpu):
    a = _tangents(64, 5).to(gpu)
    assert torch.allclose(Sim3.exp(a).log(), a, atol=1e-8)


def test_inverse(Sim3, gpu):
    X = Sim3(_elements(64, 6).to(gpu))
    assert torch.allclose((X * X.inv()).log(), torch.zeros(64, 7, dtype=F64, device=gpu), atol=1e-8)


def test_adjoint(Sim3, gpu):
    X = Sim3(_elements(64, 7).to(gpu))
    a = 0.5 * torch.randn(64, 7, dtype=F64, device=gpu)
    lhs = X * Sim3.exp(a)
    rhs = Sim3.exp(X.adj(a)) * X
    assert torch.allclose((lhs * rhs.inv()).log(), torch.zeros_like(a), atol=1e-8)


def test_act_matches_matrix(Sim3, gpu):
    X = Sim3(_elements(64, 8).to(gpu))
    p = torch.randn(64, 3, dtype=F64, device=gpu)
    ph = torch.cat([p, torch.ones_like(p[:, :1])], 1)
    via_matrix = (X.matrix() @ ph[..., None])[..., 0]
    assert torch.allclose(X.act(p), via_matrix[:, :3], atol=1e-8)
    assert torch.allclose(X.act(ph), via_matrix, atol=1e-8)


def test_constructors(Sim3, gpu):
    from dpvo_amd.lietorch import SE3, SO3, cat, stack

    G = SE3.Random(5, device=gpu, dtype=F64)
    S = Sim3(G)
    assert S.data.shape == (5, 8) and torch.equal(S.data[:, 7], torch.ones(5, dtype=F64, device=gpu))
    assert torch.equal(S.data[:, :7], G.data)
    Q = Sim3(SO3.Random(5, device=gpu, dtype=F64))
    assert torch.equal(Q.data[:, :3], torch.zeros(5, 3, dtype=F64, device=gpu))
    assert torch.equal(Q.data[:, 7], torch.ones(5, dtype=F64, device=gpu))
    assert torch.equal(Sim3(S).data, S.data)
    I = Sim3.Identity(2, 3, device=gpu, dtype=F64)
    assert I.shape == (2, 3)
    assert torch.allclose(I.matrix(), torch.eye(4, dtype=F64, device=gpu).expand(2, 3, 4, 4), atol=1e-15)
    X = Sim3.Random(4, device=gpu, dtype=F64)
    assert X.data.shape == (4, 8) and X.log().shape == (4, 7)
    assert cat([X, S], 0).data.shape == (9, 8) and stack([X, X], 0).data.shape == (2, 4, 8)
    assert torch.allclose(X.retr(torch.zeros(4, 7, dtype=F64, device=gpu)).data, X.data, atol=1e-14)
    assert torch.equal(Sim3.InitFromVec(X.data).data, X.data)
    assert torch.allclose(X.translation()[:, :3], X.data[:, :3], atol=1e-14)


# ---- gradients through the class API against the restatement's autograd ----
B = 3


def _jac(f, a):
    """Jacobian of a batched map [B, 7] -> [B, ...] as [B, out, 7]."""
    J = torch.autograd.functional.jacobian(lambda x: f(x).reshape(B, -1).sum(0), a)
    return J.permute(1, 0, 2)


def _fixed(seed, lifted=False):
    X = _elements(40, seed)[20:20 + B].clone()  # general rows, past the small-argument ones
    X[:, 3:7] /= 1.3
    if lifted:
        X[:, 7] = 1.0
    return X


def _compare(gpu, f_gpu, f_ref, a):
    got = _jac(f_gpu, a.to(gpu)).cpu()
    ref = _jac(f_ref, a)
    assert torch.isfinite(got).all()
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=1e-8)


A_POINTS = {"zero": lambda: torch.zeros(B, 7, dtype=F64),
            "half": lambda: 0.5 * torch.nn.functional.normalize(
                torch.randn(B, 7, dtype=F64, generator=torch.Generator().manual_seed(11)), dim=1)}


@pytest.mark.parametrize("at", ["zero", "half"])
def test_exp_log_grad(Sim3, gpu, at):
    _compare(gpu, lambda a: Sim3.exp(a).log(), lambda a: R.Log(R.Exp(a)), A_POINTS[at]())


@pytest.mark.parametrize("lifted", [False, True], ids=["general", "se3_lifted"])
@pytest.mark.parametrize("at", ["zero", "half"])
def test_inv_log_grad(Sim3, gpu, at, lifted):
    X = _fixed(12, lifted)
    M, Xg = R.from_data(X), Sim3(X.to(gpu))
    _compare(gpu, lambda a: (Sim3.exp(a) * Xg).inv().log(),
             lambda a: R.Log(R.inv(R.Exp(a) @ M)), A_POINTS[at]())


@pytest.mark.parametrize("transpose", [False, True], ids=["adj", "adjT"])
def test_adj_grad(Sim3, gpu, transpose):
    X = _fixed(13)
    M, Xg = R.from_data(X), Sim3(X.to(gpu))
    b = torch.randn(B, 7, dtype=F64, generator=torch.Generator().manual_seed(14))
    bg = b.to(gpu)

    def f_gpu(a):
        Y = Sim3.exp(a) * Xg
        return Y.adjT(bg) if transpose else Y.adj(bg)

    def f_ref(a):
        Ad = R.Adj_matrix(R.Exp(a) @ M)
        return ((Ad.transpose(1, 2) if transpose else Ad) @ b[..., None])[..., 0]

    _compare(gpu, f_gpu, f_ref, A_POINTS["zero"]())
    # and with respect to b
    a0 = A_POINTS["half"]()
    Yg, Ad = Sim3.exp(a0.to(gpu)) * Xg, R.Adj_matrix(R.Exp(a0) @ M)
    _compare(gpu, (lambda v: Yg.adjT(v)) if transpose else (lambda v: Yg.adj(v)),
             lambda v: ((Ad.transpose(1, 2) if transpose else Ad) @ v[..., None])[..., 0], b)


@pytest.mark.parametrize("dim", [3, 4])
def test_act_grad(Sim3, gpu, dim):
    X = _fixed(15)
    M, Xg = R.from_data(X), Sim3(X.to(gpu))
    p = torch.randn(B, dim, dtype=F64, generator=torch.Generator().manual_seed(16))
    pg = p.to(gpu)

    def ref_act(Y, v):
        if dim == 3:
            return (Y[:, :3, :3] @ v[..., None])[..., 0] + Y[:, :3, 3]
        return (Y @ v[..., None])[..., 0]

    for at in ("zero", "half"):
        _compare(gpu, lambda a: (Xg * Sim3.exp(a)).act(pg), lambda a: ref_act(M @ R.Exp(a), p),
                 A_POINTS[at]())
    got = torch.autograd.functional.jacobian(lambda v: Xg.act(v).sum(0), pg).cpu()
    ref = torch.autograd.functional.jacobian(lambda v: ref_act(M, v).sum(0), p)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=1e-8)


@pytest.mark.parametrize("what", ["matrix", "translation", "vec"])
def test_matrix_translation_vec_grad(Sim3, gpu, what):
    X = _fixed(17)
    X[:, 3:6] *= 0.3  # keeps qw > 0 in X exp(a), the sign to_data() returns
    X[:, 3:7] /= X[:, 3:7].norm(dim=1, keepdim=True)
    M, Xg = R.from_data(X), Sim3(X.to(gpu))
    f_gpu = {"matrix": lambda a: (Xg * Sim3.exp(a)).matrix(),
             "translation": lambda a: (Xg * Sim3.exp(a)).translation(),
             "vec": lambda a: (Xg * Sim3.exp(a)).vec()}[what]
    f_ref = {"matrix": lambda a: M @ R.Exp(a),
             "translation": lambda a: (M @ R.Exp(a))[:, :, 3],
             "vec": lambda a: R.to_data(M @ R.Exp(a))}[what]
    for at in ("zero", "half"):
        a = A_POINTS[at]() * (0.4 if what == "vec" else 1.0)
        if what == "vec":
            assert torch.allclose(f_gpu(a.to(gpu)).cpu(), f_ref(a), atol=1e-12)  # same sign of q
        _compare(gpu, f_gpu, f_ref, a)


def test_transform_jacobians_with_sim3_poses(Sim3, gpu):
    """projective_ops.transform(jacobian=True) with Sim3 poses, 6 edges: Ji, Jj,
    Jz against autograd of the projected patch centre through the restatement."""
    from dpvo_amd import projective_ops as pops

    g = torch.Generator().manual_seed(21)
    nposes, E, P = 4, 6, 3
    a = 0.15 * torch.randn(nposes, 7, dtype=F64, generator=g)
    poses = R.to_data(R.Exp(a))
    ii = torch.tensor([0, 0, 1, 2, 3, 1])
    jj = torch.tensor([1, 2, 3, 0, 2, 0])
    kk = torch.tensor([0, 1, 2, 3, 4, 5])
    patches = torch.zeros(1, 6, 3, P, P, dtype=F64)
    patches[0, :, 0] = 100 + 200 * torch.rand(6, 1, 1, dtype=F64, generator=g) + torch.arange(P)[None, None, :]
    patches[0, :, 1] = 80 + 150 * torch.rand(6, 1, 1, dtype=F64, generator=g) + torch.arange(P)[None, :, None]
    patches[0, :, 2] = 0.3 + 0.4 * torch.rand(6, 1, 1, dtype=F64, generator=g)
    intr = torch.tensor([[300.0, 310.0, 240.0, 180.0]], dtype=F64).repeat(nposes, 1)[None]

    x1, valid, (Ji, Jj, Jz) = pops.transform(Sim3(poses[None].to(gpu)), patches.to(gpu),
                                             intr.to(gpu), ii.to(gpu), jj.to(gpu), kk.to(gpu),
                                             jacobian=True)
    assert Ji.shape == (1, E, 2, 7) and Jj.shape == (1, E, 2, 7) and Jz.shape == (1, E, 2, 1)
    assert bool((valid > 0.5).all())

    Mp = R.from_data(poses)
    c = P // 2
    x0 = torch.stack([(patches[0, kk, 0, c, c] - 240.0) / 300.0, (patches[0, kk, 1, c, c] - 180.0) / 310.0,
                      torch.ones(E, dtype=F64)], -1)
    d0 = patches[0, kk, 2, c, c]

    def centre(di, dj, dz):
        Gij = (R.Exp(dj) @ Mp[jj]) @ R.inv(R.Exp(di) @ Mp[ii])
        X = (Gij @ torch.cat([x0, (d0 + dz)[:, None]], -1)[..., None])[..., 0]
        return torch.stack([300.0 * X[:, 0] / X[:, 2] + 240.0, 310.0 * X[:, 1] / X[:, 2] + 180.0], -1)

    z7, z1 = torch.zeros(E, 7, dtype=F64), torch.zeros(E, dtype=F64)
    np.testing.assert_allclose(x1[0, :, c, c].cpu().numpy(), centre(z7, z7, z1).numpy(), atol=1e-9)
    Ri, Rj, Rz = torch.autograd.functional.jacobian(lambda *v: centre(*v).sum(0), (z7, z7, z1))
    np.testing.assert_allclose(Ji[0].cpu().numpy(), Ri.permute(1, 0, 2).numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(Jj[0].cpu().numpy(), Rj.permute(1, 0, 2).numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(Jz[0, :, :, 0].cpu().numpy(), Rz.permute(1, 0).numpy(), rtol=0, atol=1e-6)


def test_capi_group4_accepts_empty_batch(gpu):
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    for dtype in (0, 2):  # DPVO_F32, DPVO_F64
        assert lib.dpvo_lie_forward(4, 0, dtype, 0, None, None, None, None) == 0
        assert lib.dpvo_lie_backward(4, 0, dtype, 0, None, None, None, None, None, None) == 0
    assert lib.dpvo_pgo_residual(None, None, None, None, 0, 0, 2, None, None, None, None) == 0
