"""Loop-closure pose-graph optimisation on the device (dpvo_amd/loop_closure.py,
cuda_ba.pgo_residual) against the fp64 torch restatement of
tests/sim3_restatement.py, on a synthetic loop with scale drift.

Measured on an MI355X:
  pgo_residual against the restatement, max abs difference over res / J_i / J_j:
    f64 I/O 7e-14 (bound 1e-9); f32 I/O 1.2e-7 (bound rtol 1e-5, atol 1e-6).
  the same with residuals chosen from the (theta, sigma) grid of
  tests/sim3_bands.py (144 edges, theta <= 3, pure scalings included, values up
  to 8.6): f64 res 1.2e-14, J_i 1.1e-13, J_j 1.3e-13; f32 res 1.2e-7, J_i
  2.4e-7, J_j 1.9e-7, under the same bounds; 1, 16, 17 and 257 edges through
  the C ABI leave the rows before and after their outputs untouched.
  run_pgo, f32 poses on the device against the fp64 restatement LM:
    n = 12 / 2 loops: mean square 3.03e-2 -> 5.94e-5 (restatement 5.94e-5, 30
      iterations); re-anchored result differs by 8.3e-7 in translation, 6.1e-8
      in the quaternion, 1.0e-7 in scale; scales 1.0000 .. 1.2519.
    n = 40 / 5 loops: 2.35e-2 -> 5.33e-6 (restatement 5.33e-6, 7 iterations);
      1.5e-6 / 7.0e-8 / 2.2e-7; scales 1.0000 .. 1.2745.
  The scale-1 pose is the one next to the anchor (pose safe_i - 1, whose
  odometry edge to the anchor is met exactly: 1 +- 1e-8 measured); pose 0, at
  the far end of the drift, carries the largest scale.
"""
import math

import numpy as np
import pytest
import torch

import sim3_restatement as R

F64 = torch.float64


# ------------------------------------------------------------- synthetic loop
def _rot(axis, ang):
    c, s = math.cos(ang), math.sin(ang)
    if axis == "z":
        return torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1.0]], dtype=F64)
    return torch.tensor([[1.0, 0, 0], [0, c, -s], [0, s, c]], dtype=F64)


def make_loop(n, L):
    """n world-to-camera poses on a circle of radius 5 (start angle 0.3, so no
    pose has zero rotation), yaw following the circle plus a small roll; a bit
    more than one lap, so that poses n-L-1 .. n-2 see poses 0 .. L-1 again.
    The odometry is integrated with the translation of step k scaled by
    c_k = linspace(1, 1.3, n) (scale drift).  Loop edges ii = n-L-1 .. n-2,
    jj = 0 .. L-1 carry dS = Sim3(t = c_j t_ij, R_ij, s = c_j / c_i) from the
    undrifted geometry, (R_ij, t_ij) = G_j G_i^-1.  Returns (input_poses [n, 7],
    the inverses of the drifted poses; dSloop [L, 8]; ii; jj), fp64."""
    G = []
    for k in range(n):
        al = 0.3 + 2 * math.pi * k / (n - L - 0.5)
        Rwc = _rot("z", al + math.pi / 2) @ _rot("x", 0.1 * math.sin(3 * al))
        T = torch.eye(4, dtype=F64)
        T[:3, :3] = Rwc
        T[:3, 3] = torch.tensor([5 * math.cos(al), 5 * math.sin(al), 0.0], dtype=F64)
        G.append(torch.linalg.inv(T))
    c = torch.linspace(1, 1.3, n, dtype=F64)
    P = [G[0]]
    for k in range(1, n):
        D = G[k] @ torch.linalg.inv(G[k - 1])
        D[:3, 3] *= c[k]
        P.append(D @ P[-1])
    # the optimiser takes camera-to-world poses: its variables are the tangents
    # of their inverses (optim_utils.py:221)
    poses = R.to_data(torch.linalg.inv(torch.stack(P)))[:, :7]
    ii = torch.arange(n - L - 1, n - 1)
    jj = torch.arange(0, L)
    dS = []
    for i, j in zip(ii.tolist(), jj.tolist()):
        Tij = G[j] @ torch.linalg.inv(G[i])
        M = Tij.clone()
        M[:3, :3] = (c[j] / c[i]) * Tij[:3, :3]
        M[:3, 3] = c[j] * Tij[:3, 3]
        dS.append(M)
    return poses, R.to_data(torch.stack(dS)), ii, jj


def graph_of(poses, dSloop, ii, jj):
    """Constants (4x4) and indices of the whole graph and the starting tangents,
    by the restatement (optim_utils.py:163-183, 221)."""
    n = poses.shape[0]
    T = R.inv(R.from_data(poses))
    kk = torch.arange(1, n)
    C = torch.cat([T[kk - 1] @ R.inv(T[kk]), R.from_data(dSloop)])
    return C, torch.cat([kk, ii]), torch.cat([kk - 1, jj]), R.Log(T)


def ref_perform_updates(poses, dSloop, ii, jj, iters, ep=0.0, lmbda=1e-6):
    """The reference's LM (optim_utils.py:211-243) on the restatement with a
    dense fp64 solve.  Returns (final 4x4 [n], mean-square history)."""
    C, iii, jjj, Ginv = graph_of(poses, dSloop, ii, jj)
    n, r = Ginv.shape[0], len(iii)
    ms = lambda g: R.pgo_residual(C, g[iii], g[jjj]).square().mean().item()  # noqa: E731
    hist = []
    for itr in range(iters):
        res = R.pgo_residual(C, Ginv[iii], Ginv[jjj])
        Ji, Jj = R.pgo_jacobians(C, Ginv[iii], Ginv[jjj])
        hist.append(res.square().mean().item())
        J = torch.zeros(r, 7, n, 7, dtype=F64)
        e = torch.arange(r)
        J[e, :, iii] = Ji
        J[e, :, jjj] = Jj
        J = J.reshape(7 * r, 7 * n)
        A = J.T @ J
        d = A.diagonal().clone()
        A.diagonal().add_(d * lmbda + ep)
        delta = torch.linalg.solve(A, -(J.T @ res.reshape(-1))).reshape(n, 7)
        if ms(Ginv + delta) < hist[-1]:
            Ginv = Ginv + delta
            lmbda /= 2
        else:
            lmbda *= 2
        if hist[-1] < 1e-5 and itr >= 4 and hist[-5] / hist[-1] < 1.5:
            break
    return R.inv(R.Exp(Ginv)), hist


def ref_run_pgo(poses, dSloop, ii, jj, iters=30):
    """(re-anchored result [safe_i] as 4x4, the LM's own result [n], history)."""
    final, hist = ref_perform_updates(poses, dSloop, ii, jj, iters)
    s = int(ii.max()) + 1
    anchored = (R.from_data(poses)[s] @ R.inv(final[s])) @ final
    return anchored[:s], final, hist


_REF = {}


def reference(n, L):
    """The loop and the restatement LM's result, computed once per size."""
    if (n, L) not in _REF:
        loop = make_loop(n, L)
        _REF[(n, L)] = (loop,) + ref_run_pgo(*loop)
    return _REF[(n, L)]


# ---------------------------------------------------------------- CPU: oracle
def test_restatement_checks_itself():
    """No GPU: Exp / Log round trip of the restatement, and its autograd
    Jacobian of the pose-graph residual against central differences, for
    general edges and for a pure-translation residual at sigma = theta = 0."""
    g = torch.Generator().manual_seed(0)
    a = torch.randn(32, 7, dtype=F64, generator=g)
    a[:, 3:6] *= 0.8
    a[:, 6] *= 0.3
    a[0, 3:] = 0
    a[1] = 0
    M = R.Exp(a)
    assert (R.Exp(R.Log(M)) - M).abs().max() < 1e-12
    assert (R.Log(M) - a).abs().max() < 1e-12
    assert (R.from_data(R.to_data(M)) - M).abs().max() < 1e-12

    r = 6
    C = R.Exp(0.5 * torch.randn(r, 7, dtype=F64, generator=g))
    gi = 0.5 * torch.randn(r, 7, dtype=F64, generator=g)
    gj = 0.5 * torch.randn(r, 7, dtype=F64, generator=g)
    C[0] = R.from_data(torch.tensor([0.3, -0.2, 0.1, 0, 0, 0, 1, 1], dtype=F64))
    gi[0] = 0
    gj[0] = 0
    res = R.pgo_residual(C, gi, gj)
    assert torch.allclose(res[0], torch.tensor([0.3, -0.2, 0.1, 0, 0, 0, 0], dtype=F64), atol=1e-15)
    Ji, Jj = R.pgo_jacobians(C, gi, gj)
    assert torch.isfinite(Ji).all() and torch.isfinite(Jj).all()
    for h in (1e-6, 1e-7):
        for k in range(7):
            d = torch.zeros(7, dtype=F64)
            d[k] = h
            fi = (R.pgo_residual(C, gi + d, gj) - R.pgo_residual(C, gi - d, gj)) / (2 * h)
            fj = (R.pgo_residual(C, gi, gj + d) - R.pgo_residual(C, gi, gj - d)) / (2 * h)
            assert (fi - Ji[:, :, k]).abs().max() < 1e-7
            assert (fj - Jj[:, :, k]).abs().max() < 1e-7


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    return dpvo_amd.load_extension("cuda_ba")


def _edge_inputs(case):
    """(Ginv [n, 7], C data [r, 8], iii, jjj) in fp64."""
    if case in ("start", "perturbed"):
        poses, dS, ii, jj = make_loop(12, 2)
    else:
        poses, dS, ii, jj = make_loop(200, 8)
    C, iii, jjj, Ginv = graph_of(poses, dS, ii, jj)
    Cd = R.to_data(C)
    if case == "start":
        # one more edge whose residual is the pure translation (0.3, -0.2, 0.1):
        # zero rotation and zero log-scale, where a constant small-angle branch shows
        Ginv = torch.cat([Ginv, torch.zeros(2, 7, dtype=F64)])
        Cd = torch.cat([Cd, torch.tensor([[0.3, -0.2, 0.1, 0, 0, 0, 1, 1]], dtype=F64)])
        iii = torch.cat([iii, torch.tensor([12])])
        jjj = torch.cat([jjj, torch.tensor([13])])
    elif case == "perturbed":
        Ginv = Ginv + 0.05 * torch.randn(Ginv.shape, dtype=F64, generator=torch.Generator().manual_seed(1))
    else:
        Ginv = Ginv + 0.02 * torch.randn(Ginv.shape, dtype=F64, generator=torch.Generator().manual_seed(2))
        assert len(iii) == 207
    return Ginv, Cd, iii, jjj


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["start", "perturbed", "r207"])
def test_pgo_residual_matches_restatement(cb, gpu, case, dtype):
    Ginv, Cd, iii, jjj = _edge_inputs(case)
    Gd, Cdd = Ginv.to(gpu, dtype), Cd.to(gpu, dtype)
    res, Ji, Jj = cb.pgo_residual(Gd, Cdd, iii.to(gpu), jjj.to(gpu), True)
    r = len(iii)
    assert res.shape == (r, 7) and Ji.shape == (r, 7, 7) and Jj.shape == (r, 7, 7)
    assert res.dtype == dtype and Ji.dtype == dtype and Jj.dtype == dtype
    # both sides compute in fp64 from the same (rounded) inputs
    G64, C64 = Gd.double().cpu(), R.from_data(Cdd.double().cpu())
    rres = R.pgo_residual(C64, G64[iii], G64[jjj])
    rJi, rJj = R.pgo_jacobians(C64, G64[iii], G64[jjj])
    tol = dict(rtol=0, atol=1e-9) if dtype == torch.float64 else dict(rtol=1e-5, atol=1e-6)
    for name, got, ref in (("res", res, rres), ("J_i", Ji, rJi), ("J_j", Jj, rJj)):
        got = got.double().cpu()
        assert torch.isfinite(got).all(), name
        print(case, dtype, name, "max abs diff", (got - ref).abs().max().item())
        np.testing.assert_allclose(got.numpy(), ref.numpy(), err_msg=name, **tol)
    if case == "start":
        chain = res[:11].double().cpu()
        assert chain.abs().max() < (1e-12 if dtype == torch.float64 else 1e-5)  # odometry edges: 0
        assert torch.allclose(res[-1].double().cpu(),
                              torch.tensor([0.3, -0.2, 0.1, 0, 0, 0, 0], dtype=F64), atol=1e-6)
    # jacobian=False: the same residual, bit for bit
    only, = cb.pgo_residual(Gd, Cdd, iii.to(gpu), jjj.to(gpu), False)
    assert torch.equal(only, res)


# ---- residuals chosen from the (theta, sigma) grid of tests/sim3_bands.py ----
def band_edges(res, seed, zero_every=4):
    """Edges whose residual is the given tangent: gi, gj ~ 0.5 N(0, 1) (every
    `zero_every`-th edge: gi = gj = 0) and C = Exp(res) Exp(gj) Exp(gi)^-1, so
    that Log(C Exp(gi) Exp(gj)^-1) = res.  C goes to data by a conversion that
    is right for any rotation (R.to_data needs w > 0).  Returns (Ginv [2m, 7],
    C data [m, 8], iii, jjj), fp64; edge e joins poses e and m + e."""
    import sim3_bands as B

    m = len(res)
    g = torch.Generator().manual_seed(seed)
    gi = 0.5 * torch.randn(m, 7, dtype=F64, generator=g)
    gj = 0.5 * torch.randn(m, 7, dtype=F64, generator=g)
    gi[::zero_every] = 0
    gj[::zero_every] = 0
    C = R.Exp(res) @ R.Exp(gj) @ R.inv(R.Exp(gi))
    Cd = B.to_data(C)
    Cd[1::2, 3:7] *= -1  # either sign of the quaternion
    return torch.cat([gi, gj]), Cd, torch.arange(m), m + torch.arange(m)


_BANDS = {}


def band_case(name, dtype):
    """(Ginv, C data, iii, jjj rounded to dtype as fp64; chosen residual; the
    restatement's res, J_i, J_j at the rounded inputs), computed once."""
    import sim3_bands as B

    if (name, dtype) not in _BANDS:
        if name == "grid":  # every (theta <= 3, sigma) point, pure scalings included
            res, _ = B.grid_tangents(B.THETA[:12], per=1, seed=60)
            assert len(res) == 144
            # with zero_every = 5 the gi = gj = 0 edges fall on every sigma column
            Ginv, Cd, iii, jjj = band_edges(res, 61, zero_every=5)
        else:  # r edges cycling through a handful of grid points, one per regime
            pts = [(0.0, 0.501), (0.0, -0.499), (0.0499, 0.501), (0.0501, -0.499), (0.0199, 3.0),
                   (0.0201, -2.0), (3.0, 0.499), (1e-9, 1e-9), (2.0, -0.501)]
            r = int(name[1:])
            res, _ = B.tangents_at([pts[k % len(pts)] for k in range(r)], 1, 62 + r)
            Ginv, Cd, iii, jjj = band_edges(res, 63 + r)
        Ginv, Cd = Ginv.to(dtype).double(), Cd.to(dtype).double()
        C64 = R.from_data(Cd)
        rres = R.pgo_residual(C64, Ginv[iii], Ginv[jjj])
        rJi, rJj = R.pgo_jacobians(C64, Ginv[iii], Ginv[jjj])
        assert torch.isfinite(rres).all() and torch.isfinite(rJi).all() and torch.isfinite(rJj).all()
        _BANDS[(name, dtype)] = (Ginv, Cd, iii, jjj, res, rres, rJi, rJj)
    return _BANDS[(name, dtype)]


def _band_tol(dtype):
    return dict(rtol=0, atol=1e-9) if dtype == torch.float64 else dict(rtol=1e-5, atol=1e-6)


def test_band_edges_have_the_chosen_residual():
    """No GPU: the construction above, in the restatement, pure scalings included."""
    Ginv, Cd, iii, jjj, res, rres, rJi, rJj = band_case("grid", torch.float64)
    assert int(((res[:, 3:6].norm(dim=1) == 0) & (res[:, 6].abs() >= 0.499)).sum()) == 7
    assert int((Cd[:, 6] < 0).sum()) > 0  # quaternions of either sign reach the kernel
    assert float((rres - res).abs().max()) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_pgo_residual_at_the_bands(cb, gpu, dtype):
    """Residuals walking theta through 0.02 and 0.05 and sigma through +-0.5,
    with general and with zero pose tangents."""
    Ginv, Cd, iii, jjj, _, rres, rJi, rJj = band_case("grid", dtype)
    Gd, Cdd, ig, jg = Ginv.to(gpu, dtype), Cd.to(gpu, dtype), iii.to(gpu), jjj.to(gpu)
    res, Ji, Jj = cb.pgo_residual(Gd, Cdd, ig, jg, True)
    for name, got, ref in (("res", res, rres), ("J_i", Ji, rJi), ("J_j", Jj, rJj)):
        assert got.dtype == dtype and got.shape == ref.shape
        got = got.double().cpu()
        assert torch.isfinite(got).all(), name
        print("bands", dtype, name, "max abs diff", (got - ref).abs().max().item(),
              "max abs", ref.abs().max().item())
        np.testing.assert_allclose(got.numpy(), ref.numpy(), err_msg=name, **_band_tol(dtype))
    only, = cb.pgo_residual(Gd, Cdd, ig, jg, False)
    assert torch.equal(only, res)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("r", [1, 16, 17, 257])
def test_pgo_residual_edge_counts_and_guard_rows(gpu, r, dtype):
    """The Jacobian kernel takes 16 edges per 256-thread block (16 lanes per
    edge), the residual-only kernel 256: one edge, a full block, one more, and
    one more than a block of the residual-only kernel.  Through the C ABI into
    caller-owned buffers with a sentinel row on either side."""
    import ctypes

    import dpvo_amd

    lib = dpvo_amd.c_abi()
    Ginv, Cd, iii, jjj, _, rres, rJi, rJj = band_case(f"r{r}", dtype)
    Gd, Cdd, ig, jg = Ginv.to(gpu, dtype), Cd.to(gpu, dtype), iii.to(gpu), jjj.to(gpu)
    sentinel = -777.0
    buf = {k: torch.full((r + 2, w), sentinel, dtype=dtype, device=gpu)
           for k, w in (("res", 7), ("Ji", 49), ("Jj", 49), ("only", 7))}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    code = 2 if dtype == torch.float64 else 0  # DPVO_F64 / DPVO_F32
    torch.cuda.synchronize(gpu)
    null = ctypes.c_void_p(None)
    with torch.cuda.device(gpu):
        st = lib.dpvo_pgo_residual(ptr(Gd), ptr(Cdd), ptr(ig), ptr(jg), r, len(Ginv), code,
                                   ptr(buf["res"][1:]), ptr(buf["Ji"][1:]), ptr(buf["Jj"][1:]), null)
        assert st == 0
        st = lib.dpvo_pgo_residual(ptr(Gd), ptr(Cdd), ptr(ig), ptr(jg), r, len(Ginv), code,
                                   ptr(buf["only"][1:]), null, null, null)
        assert st == 0
    torch.cuda.synchronize(gpu)
    for k, t in buf.items():
        assert bool((t[0] == sentinel).all()) and bool((t[r + 1] == sentinel).all()), k
    for name, got, ref in (("res", buf["res"], rres), ("J_i", buf["Ji"], rJi), ("J_j", buf["Jj"], rJj)):
        got = got[1:r + 1].double().cpu().reshape(ref.shape)
        np.testing.assert_allclose(got.numpy(), ref.numpy(), err_msg=name, **_band_tol(dtype))
    assert torch.equal(buf["only"], buf["res"])


@pytest.mark.gpu
def test_pgo_residual_validation(cb, gpu):
    from dpvo_amd import loop_closure as lc

    n, r = 5, 3
    G = torch.zeros(n, 7, device=gpu)
    C = torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1.0]], device=gpu).repeat(r, 1)
    ii = torch.tensor([1, 2, 3], device=gpu)
    jj = torch.tensor([0, 1, 2], device=gpu)
    assert cb.pgo_residual(G, C, ii, jj, True)[0].abs().max() == 0
    bad = ii.clone()
    bad[1] = n
    with pytest.raises(RuntimeError, match="out of range"):
        cb.pgo_residual(G, C, bad, jj, True)
    with pytest.raises(RuntimeError, match="out of range"):
        cb.pgo_residual(G, C, ii, bad - n - 1, False)  # negative
    with pytest.raises(RuntimeError, match="dtype"):
        cb.pgo_residual(G, C.double(), ii, jj, True)
    with pytest.raises(RuntimeError):
        cb.pgo_residual(G, C, ii.int(), jj, True)
    with pytest.raises(RuntimeError):
        cb.pgo_residual(G[:, :6], C, ii, jj, True)
    e = torch.zeros(0, dtype=torch.long, device=gpu)
    res, Ji, Jj = cb.pgo_residual(G, C[:0], e, e, True)
    assert res.shape == (0, 7) and Ji.shape == (0, 7, 7) and Jj.shape == (0, 7, 7)
    assert cb.pgo_residual(G, C[:0], e, e, False)[0].shape == (0, 7)
    # run_pgo needs a pose after the loop to anchor the result
    poses, dS, lii, ljj = [t.to(gpu) for t in make_loop(12, 2)]
    with pytest.raises(ValueError, match="n - 1"):
        lc.run_pgo(poses.float(), dS.float(), lii + 1, ljj)


@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(12, 2), (40, 5)])
def test_run_pgo_end_to_end(gpu, n, L):
    """f32 poses on the device against the fp64 restatement LM."""
    from dpvo_amd import loop_closure as lc
    from dpvo_amd.lietorch import SE3, Sim3

    (poses, dS, ii, jj), ref_final, ref_lm, ref_hist = reference(n, L)
    C, iii, jjj, _ = graph_of(poses, dS, ii, jj)
    ms = lambda F: R.pgo_residual(C, R.Log(R.inv(F))[iii], R.Log(R.inv(F))[jjj]).square().mean().item()  # noqa: E731
    pg, dg, ig, jg = poses.to(gpu).float(), dS.to(gpu).float(), ii.to(gpu), jj.to(gpu)

    est = lc.perform_updates(pg, dg, ig, jg, iters=30)
    assert isinstance(est, Sim3) and est.data.shape == (n, 8)
    got_ms = ms(R.from_data(est.data.double().cpu()))
    ref_ms = ms(ref_lm)
    print(f"n={n} L={L}: initial {ref_hist[0]:.3e} restatement final {ref_ms:.3e} "
          f"({len(ref_hist)} iterations) device final {got_ms:.3e}")
    assert got_ms <= 1.05 * ref_ms
    assert got_ms <= 1e-2 * ref_hist[0]

    out = lc.run_pgo(pg, dg, ig, jg, iters=30)
    s = int(ii.max()) + 1
    assert out.shape == (s, 8) and out.dtype == torch.float32
    got, ref = out.double().cpu(), R.to_data(ref_final)
    dt = (got[:, :3] - ref[:, :3]).abs().max().item()
    dq = torch.minimum((got[:, 3:7] - ref[:, 3:7]).abs().amax(1),
                       (got[:, 3:7] + ref[:, 3:7]).abs().amax(1)).max().item()
    dsc = (got[:, 7] - ref[:, 7]).abs().max().item()
    print(f"n={n} L={L}: re-anchored max diff translation {dt:.3e} quaternion {dq:.3e} scale {dsc:.3e}; "
          f"scales {got[:, 7].min().item():.4f} .. {got[:, 7].max().item():.4f}, "
          f"pose 0 {got[0, 7].item():.7f}, pose {s - 1} {got[s - 1, 7].item():.8f}")
    assert dt <= 1e-4 and dq <= 1e-4 and dsc <= 1e-5
    # the pose next to the anchor keeps the anchor's scale 1 (its odometry edge
    # is met exactly); the scale grows towards pose 0, the far end of the drift
    assert abs(got[s - 1, 7].item() - 1.0) <= 1e-6
    assert 1.2 <= got[:, 7].max().item() <= 1.3

    # split_result: the SE3 to store and the depth divisor
    inv7, scale = lc.split_result(out)
    assert inv7.shape == (s, 7) and scale.shape == (s,)
    assert torch.equal(scale, out[:, 7])
    p = torch.randn(s, 3, device=gpu)
    # X^-1 p = R^T (p - t) / s: the SE3 carries R^T (p - t), the scale goes to the depths
    Xinv = Sim3(out).inv()
    assert torch.allclose(SE3(inv7).act(p), scale[:, None] * Xinv.act(p), atol=1e-5)
    assert torch.allclose(inv7[:, 3:], Xinv.data[:, 3:7], atol=1e-6)
