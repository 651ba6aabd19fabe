"""GPU: the fused BA layer (dpvo_amd.ba.BA over ba_layer.hip) against the
fp64 restatement of ba_layer_ref on the same values: outputs and all four
gradients for a random cotangent, per tensor as max-abs error over max-abs of
the reference, for poses also per pose row.

fp64 bound: the largest deviation over all cases measured on the first MI355X
run was 4.02e-11 (the weight gradient of case a_p1; DESIGN.md lists the
largest per tensor); the bound is 100 x that, to absorb
summation order, and stays below the 1e-8 that test_sim3_gpu.py applies to
fp64 derivatives.  The two window cases whose pose system leaves small LDS
(ba_layer_ref.WINDOW_CASES) take max(that bound, 100 x their own
summation-order floor, measured from the restatement alone: order_floor).
fp32 bound: 2 x the deviation of the restatement run in
fp32 from its fp64 run on that case and tensor, computed here.
"""
import functools

import pytest
import torch

import ba_layer_ref as R

pytestmark = pytest.mark.gpu

FP64_BOUND = 100 * 4.02e-11
assert FP64_BOUND < 1e-8
TENSORS = ("poses", "patches", "g_poses", "g_patches", "g_targets", "g_weights")
DT = {"f64": torch.float64, "f32": torch.float32}


@functools.lru_cache(maxsize=None)
def reference(name, values, dtype, chain=1):
    """The restatement on the case's values rounded to `values`, run in `dtype`."""
    c = R.case(name)
    r = lambda x: x.to(DT[values]).double()  # noqa: E731
    c = c.replace(name, poses=r(c.poses), patches=r(c.patches), intr=r(c.intr), targets=r(c.targets),
                  weights=r(c.weights))
    return R.ref_grads(c, R.cotangents(c), DT[dtype], chain)


def layer(c, dtype, dev, chain=1, num_poses=True, status=False, cot=None):
    from dpvo_amd.ba import BA
    from dpvo_amd.lietorch import SE3

    cot = cot or R.cotangents(c)
    d = lambda x: x.to(dtype).to(dev)  # noqa: E731
    P, K, T, W = (d(x)[None].requires_grad_() for x in (c.poses, c.patches, c.targets, c.weights))
    intr = d(c.intr)[None]
    ii, jj, kk = c.ii.to(dev), c.jj.to(dev), c.kk.to(dev)
    poses, k, st = SE3(P), K, None
    for _ in range(chain):
        out = BA(poses, k, intr, T, W, c.lmbda, ii, jj, kk, c.bounds, ep=c.ep, fixedp=c.fixedp,
                 structure_only=c.structure_only, num_poses=c.n if num_poses else None,
                 return_status=True)
        poses, k, st = out
    moved = SE3(poses.data[:, :, None]).act(d(cot["pts"])[None])
    loss = (d(cot["cP"]) * moved).sum() + (d(cot["cK"]) * k).sum()
    loss.backward()
    res = {"poses": poses.data[0], "patches": k[0], "g_poses": P.grad[0, :, :6],
           "g_patches": K.grad[0], "g_targets": T.grad[0], "g_weights": W.grad[0],
           "g_pad": P.grad[0, :, 6]}
    res = {k_: v.detach().double().cpu() for k_, v in res.items()}
    if status:
        res["status"] = st.cpu().tolist()
    return res


def rel(got, ref):
    s = ref.abs().max()
    if s == 0:
        return 0.0 if got.abs().max() == 0 else float("inf")
    return float((got - ref).abs().max() / s)


def deviations(got, ref):
    """name -> deviation, poses and their gradient also per row."""
    out = {t: rel(got[t], ref[t]) for t in TENSORS}
    for t in ("poses", "g_poses"):
        out[t + "/row"] = max(rel(got[t][i], ref[t][i]) for i in range(ref[t].shape[0]))
    return out


@functools.lru_cache(maxsize=None)
def order_floor(name):
    """Summation-order noise of the case, from the reference alone: the
    deviation per tensor between two fp64 runs of the restatement, edges in the
    given order and under one fixed permutation (outputs un-permuted)."""
    c = R.case(name)
    cp, perm = R.permuted(c)
    other = dict(R.ref_grads(cp, R.cotangents(c)))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    for t in ("g_targets", "g_weights"):
        other[t] = other[t][inv]
    return deviations(other, reference(name, "f64", "f64"))


def check(name, dtype, dev, chain=1, floor=False):
    """floor: the fp64 bound is max(FP64_BOUND, 100 x order_floor(name))."""
    c = R.case(name)
    got = layer(c, DT[dtype], dev, chain)
    ref = reference(name, dtype, "f64", chain)
    dev_ = deviations(got, ref)
    if dtype == "f64" and floor:
        fl = order_floor(name)
        print(f"\n[ba_layer] {name} floor " + " ".join(f"{t}={v:.2e}" for t, v in fl.items()))
        bound = {t: max(FP64_BOUND, 100 * fl[t]) for t in dev_}
    elif dtype == "f64":
        bound = {t: FP64_BOUND for t in dev_}
    else:
        own = deviations(reference(name, "f32", "f32", chain), ref)
        bound = {t: 2 * v for t, v in own.items()}
    print(f"\n[ba_layer] {name} {dtype} chain={chain} " +
          " ".join(f"{t}={v:.2e}/{bound[t]:.2e}" for t, v in dev_.items()))
    assert (got["g_pad"] == 0).all()
    bad = {t: (v, bound[t]) for t, v in dev_.items() if not v <= bound[t]}
    assert not bad, bad
    return got, ref


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", R.GPU_CASES)
def test_matches_restatement(gpu, name, dtype):
    check(name, dtype, gpu)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", R.WINDOW_CASES)
def test_pose_system_beyond_small_lds(gpu, name, dtype):
    """16 free poses: the 96 x 96 pose system factors in LDS above 64 KB; 24:
    the factor lives in the workspace in HBM and the backward's solve-only
    call reads it there.  Outputs and all four gradients."""
    import spd_cases as S

    nf = R.case(name).n - R.case(name).fixedp
    assert S.residency(6 * nf, 1, S.F64) == {16: S.RAISED, 24: S.HBM}[nf]
    got, ref = check(name, dtype, gpu, floor=True)
    assert not ref["aux"]["failed"] and ref["aux"]["dX"].abs().max() > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["b", "c_65"])
def test_two_chained_calls(gpu, name, dtype):
    """for itr in range(2) of net.py:509: the second call receives the first
    call's outputs, so its gradient passes through the derivative of the
    first call's Jacobians."""
    check(name, dtype, gpu, chain=2)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_two_identical_calls_are_bit_identical(gpu, dtype):
    c = R.case("g")
    a, b = layer(c, DT[dtype], gpu, chain=2), layer(c, DT[dtype], gpu, chain=2)
    for t in TENSORS:
        assert torch.equal(a[t], b[t]), t


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_failed_factorisation(gpu, dtype):
    """(h) ep = -1e6: dX = 0, the poses unchanged bit for bit, the dZ path
    keeps its gradient, the status word is set."""
    c = R.case("h")
    got, ref = check("h", dtype, gpu)
    assert ref["aux"]["failed"]
    assert torch.equal(got["poses"], c.poses.to(DT[dtype]).double())
    st = layer(c, DT[dtype], gpu, status=True)["status"]
    assert st[0] == 0 and st[1] != 0
    assert got["g_targets"].abs().max() > 0 and got["g_patches"].abs().max() > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_out_of_range_edges_are_closed(gpu, dtype):
    """(i) kk = M and jj = -1, out by one: equal to the case without them."""
    c = R.case("c_63")
    M = c.patches.shape[0]
    L = torch.tensor
    ci = c.replace("i", ii=torch.cat([c.ii, L([1, 2])]), jj=torch.cat([c.jj, L([2, -1])]),
                   kk=torch.cat([c.kk, L([M, 3])]),
                   targets=torch.cat([c.targets, c.targets[:2]]),
                   weights=torch.cat([c.weights, c.weights[:2]]))
    ci.n = c.n
    got = layer(ci, DT[dtype], gpu, status=True)
    base = layer(c, DT[dtype], gpu, status=True)
    assert got["status"][0] == 2 and base["status"][0] == 0
    for t in ("poses", "patches", "g_poses", "g_patches"):
        assert torch.equal(got[t], base[t]), t
    for t in ("g_targets", "g_weights"):
        assert torch.equal(got[t][:-2], base[t]) and (got[t][-2:] == 0).all(), t


def test_no_host_synchronisation(gpu):
    c = R.case("c_257")
    layer(c, torch.float32, gpu)  # warm-up: library load, LDS attribute
    from dpvo_amd.ba import BA
    from dpvo_amd.lietorch import SE3

    P, K, T, W = (x.float().to(gpu)[None].requires_grad_()
                  for x in (c.poses, c.patches, c.targets, c.weights))
    intr, ii, jj, kk = c.intr.float().to(gpu)[None], c.ii.to(gpu), c.jj.to(gpu), c.kk.to(gpu)
    lm = torch.full((1,), 1e-4, device=gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        poses, k = BA(SE3(P), K, intr, T, W, lm, ii, jj, kk, c.bounds, ep=c.ep, fixedp=c.fixedp,
                      num_poses=c.n)
        (poses.data.sum() + k.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(P.grad).all() and P.grad.abs().max() > 0


def test_num_poses_none_and_print(gpu, capsys):
    """num_poses=None computes n as the reference does (one sync): the same
    bits as with n given; PRINT=True prints the mean gated residual."""
    from dpvo_amd.ba import BA
    from dpvo_amd.lietorch import SE3

    c = R.case("e")
    d = lambda x: x.to(gpu)[None]  # noqa: E731
    args = (SE3(d(c.poses)), d(c.patches), d(c.intr), d(c.targets), d(c.weights), c.lmbda,
            c.ii.to(gpu), c.jj.to(gpu), c.kk.to(gpu), c.bounds)
    a = BA(*args, ep=c.ep, fixedp=c.fixedp, num_poses=c.n)
    capsys.readouterr()
    b = BA(*args, ep=c.ep, fixedp=c.fixedp, PRINT=True)
    printed = float(capsys.readouterr().out.strip())
    assert torch.equal(a[0].data, b[0].data) and torch.equal(a[1], b[1])
    aux = c.run()[2]
    want = float((aux["rnorm"] * aux["open"]).mean())
    assert abs(printed - want) <= 1e-9 * want, (printed, want)


@pytest.mark.parametrize("fx", ["ba_py_a", "ba_py_b"])
def test_python_ba_wrapper(gpu, fx):
    """The fork's per-frame call against `iterations` chained ba_step calls
    with its bounds and ep = 100, at test_cpu_baseline.py's fp64 bars."""
    import numpy as np

    import cpu_baseline
    from dpvo_amd.ba import python_ba_wrapper

    c = R.case("d_" + fx)
    Pr, Kr = c.poses, c.patches
    for _ in range(2):
        Pr, Kr = cpu_baseline.ba_step(Pr, Kr, c.intr[0], c.targets, c.weights, 1e-4, c.ii, c.jj,
                                      c.kk, c.fixedp, ep=100.0, bounds=None)
    poses, patches = c.poses.to(gpu).clone(), c.patches.to(gpu).clone()
    out = python_ba_wrapper(poses, patches, c.intr.to(gpu), c.targets.to(gpu), c.weights.to(gpu),
                            torch.tensor([1e-4], dtype=torch.float64, device=gpu), c.ii.to(gpu),
                            c.jj.to(gpu), c.kk.to(gpu), None, c.fixedp, c.n, 2)
    assert out.data_ptr() == poses.data_ptr()
    print(f"\n[ba_layer] wrapper {fx} dP={float((poses.cpu() - Pr).abs().max()):.2e} "
          f"dK={float((patches.cpu() - Kr).abs().max()):.2e}")
    np.testing.assert_allclose(poses.cpu().numpy(), Pr.numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(patches.cpu().numpy(), Kr.numpy(), rtol=1e-5, atol=1e-7)
    assert (poses.cpu() - c.poses).abs().max() > 1e-5  # a step was taken


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pose_buffer_of_4096_rows(gpu, dtype):
    """The live caller's shape: a 4096-row pose buffer, fixedp = n - 10.  The
    dense system covers the 10 free poses only and the numbers do not change."""
    from dpvo_amd.synthetic import make_dpvo_window

    G = make_dpvo_window(n=14, M=6, lifetime=8)
    c = R.Case("win", G.poses.double(), G.patches.double(), G.intrinsics.double(), G.target.double(),
               G.weight.double(), G.ii, G.jj, G.kk, fixedp=4, ep=100.0)
    assert c.n == 14
    eye = torch.zeros(4096 - 14, 7, dtype=torch.float64)
    eye[:, 6] = 1.0
    big = c.replace("winbig", poses=torch.cat([c.poses, eye]),
                    intr=torch.cat([c.intr, c.intr[:1].repeat(4096 - 14, 1)]))
    big.n = 14
    cot = R.cotangents(c)
    pad = torch.zeros(4096 - 14, 3, 3, dtype=torch.float64)
    cot_big = {"pts": torch.cat([cot["pts"], pad]), "cP": torch.cat([cot["cP"], pad]), "cK": cot["cK"]}
    a, b = layer(c, DT[dtype], gpu, cot=cot), layer(big, DT[dtype], gpu, cot=cot_big)
    assert torch.equal(b["poses"][:14], a["poses"]) and torch.equal(b["poses"][14:], eye)
    assert torch.equal(b["g_poses"][:14], a["g_poses"])
    for t in ("patches", "g_patches", "g_targets", "g_weights"):
        assert torch.equal(a[t], b[t]), t
    assert a["g_poses"].abs().max() > 0
