"""GPU: the three F-BA solvers (ba_window.hip, ba.hip under select_path(2),
ba_large.hip) on the gated cases of tests/ba_gates.py against oracle.ba.

The cases close edges by each gate of the edge linearisation (|r| >= 128,
Z <= 0.2 with rho = 0 below 0.2 and points behind the camera, reprojection
outside the 64 px margin), hold edges at 100..128 px that stay open, weights
that are exactly 0, a patch and a pose whose every edge is closed, and
inverse depths that the retraction wraps at 20 and clamps at 1e-4 in each of
the two iterations; tests/test_oracle_ba_gates.py asserts all that on the CPU
and pins the oracle's gate to an fp64 restatement.

Bars: conftest.assert_ba_rel (dP, dZ, dX at 1e-4 relative), poses 2e-5 abs,
inverse depths 1e-4 rel + 1e-5, patch x / y and fixed poses bit-equal,
check_status == 0 (gating is no error), and new here: ba_gates.assert_per_pose
(every free pose's step at 1e-4 of max(its reference step, ||dXr|| / sqrt N)),
the dead patch's depth bit-unchanged, the patches the last iteration clamps
bit-equal to float32(1e-4) and the ones it wraps bit-equal to 1.

measured on an MI355X, 1 / 2 iterations (worst = largest per-pose ratio;
cond(S) of the gated system entering iteration 1 / 2, from the CPU test):
  path         case    dP               dZ               dX               worst            cond(S)
  window       cfg1    0      / 4.2e-7  3.9e-9 / 2.5e-7  1.5e-9 / 4.4e-7  2.5e-9 / 8.6e-7  1.3e5 / 1.5e6
  window       cfg2    0      / 1.0e-6  6.1e-9 / 4.8e-8  1.5e-8 / 2.1e-7  2.6e-8 / 5.8e-7  1.3e6 / 1.3e6
  window       n16     1.2e-8 / 1.0e-6  3.7e-9 / 4.0e-8  5.4e-8 / 5.3e-7  9.1e-8 / 7.1e-7  1.9e5 / 3.6e5
  window       dpvo10  0      / 0       6e-11  / 4e-11   3e-13  / 5e-10   5e-13  / 1e-9    2.2e2 / 2.2e2
  multikernel  cfg1    0      / 0       0      / 0       5e-12  / 2e-11   8e-12  / 3e-11   as window
  multikernel  cfg2    0      / 0       0      / 0       3e-13  / 1e-11   6e-13  / 2e-11   as window
  large        cfg4s   4.0e-7 / 9.6e-7  0      / 2.3e-6  4e-12  / 8.9e-7  5e-12  / 7.3e-6  5.6e5 / 6.3e6
  structure    cfg1    -                0      / 0       -                -                -
The window solve (fp32 Cholesky + one fp64 refinement step) holds the per-pose
bar with two decades to spare at cond(S) = 1.5e6, dead pose included.

With the gate or the wrap broken by hand in a scratch build, these 20 tests
against the 85 BA tests from before (test_ba_gpu, test_ba_window_gpu,
test_ba_large_gpu, test_ba_window_solve_sizes_gpu without full-size cfg4):
  lin_edge `< 128.0f` -> `<= 1e9f`                      18 fail here, 85 pass there
  lin_edge `(double)Z > 0.2` -> `> 0.0`                 14 fail here, 85 pass there
  `d > 20` -> `d > 2000`: ba_window.hip final copies,
      ba.hip, ba_large.hip                              18 fail here, 85 pass there
  ba_window.hip copy between iterations (same change)   the four window x2 cases fail here,
                                                        the window tests there pass
The low clamp needs no new case in ba.hip and ba_large.hip: with 1e-4 -> 1e-5
there, 14 of the tests from before fail already (the benign cfg1, cfg2 and
cfg4s graphs hold patches whose step ends below 1e-4)."""
import numpy as np
import pytest
import torch

import ba_gates as B
from conftest import REL_TOL, assert_ba_rel, rel_err

pytestmark = pytest.mark.gpu

# case -> the solver it reaches (asserted through plan_supported / max_free_poses below)
WINDOW = ["cfg1", "cfg2", "n16", "dpvo10"]


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    m = dpvo_amd.load_extension("cuda_ba")
    m.check_status(torch.zeros(1, device=gpu))  # clean slate
    return m


@pytest.fixture
def multikernel(cb):
    cb.select_path(2)
    yield
    cb.select_path(0)


def _forward(cb, G, gpu, t0, t1, iters, eff=False):
    D = G.to(gpu)
    poses, patches = D.poses.clone(), D.patches.clone()
    dX = cb.forward_dx(poses, patches, D.intrinsics, D.target, D.weight,
                       torch.tensor([B.LM], device=gpu), D.ii, D.jj, D.kk, G.M, t0, t1, iters, eff)
    assert cb.check_status(poses) == 0  # closed edges, empty blocks and clamps are no error
    return poses.cpu().numpy(), patches.cpu().numpy(), dX.cpu().numpy()


def _check(name, P, K, dX, iters, label):
    G, info, t0, t1 = B.case(name)
    st = B.oracle_states(name)
    P0, K0 = st[0][0], st[0][1]
    Pr, Kr, d = st[iters]
    if t1 > t0:
        e = assert_ba_rel(P, K, Pr, Kr, P0, K0, t0, t1, dX, d["dX"])
        ratio = B.per_pose_ratio(dX, d["dX"])
        print(f"{label} {name} x{iters}: dP {e['dP']:.2e} dZ {e['dZ']:.2e} dX {e['dX']:.2e} "
              f"worst pose {ratio.max():.2e}")
        B.assert_per_pose(dX, d["dX"])
    else:
        e = rel_err(K[:, 2] - K0[:, 2], Kr[:, 2] - K0[:, 2])
        print(f"{label} {name} x{iters}: dZ {e:.2e}")
        assert e <= REL_TOL
        np.testing.assert_array_equal(P, P0)
    np.testing.assert_allclose(P, Pr, rtol=0, atol=2e-5)
    np.testing.assert_allclose(K[:, 2], Kr[:, 2], rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(K[:, :2], K0[:, :2])  # x, y never change
    np.testing.assert_array_equal(P[:t0], P0[:t0])      # fixed poses untouched
    np.testing.assert_array_equal(P[t1:], P0[t1:])
    if info["dead_patch"] is not None:
        np.testing.assert_array_equal(K[info["dead_patch"], 2], K0[info["dead_patch"], 2])
    if info["dead_pose"] is not None and t1 > t0:
        assert not d["dX"][info["dead_pose"] - t0].any()  # held to the floor by assert_per_pose
    wrap, low, _ = B.retraction_sets(G, st, iters)
    assert wrap.size >= 3 and low.size >= 8
    np.testing.assert_array_equal(K[wrap, 2], np.float32(1.0))
    np.testing.assert_array_equal(K[low, 2], np.float32(1e-4))


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("name", WINDOW)
def test_window_gated(cb, gpu, name, iters):
    """ba_window.hip: cfg1 shape (single-workgroup plan, E <= 512; dead pose and
    dead patch), cfg2 shape (sharded plan; dead pose), N = 16 (left-over solve
    columns), DPVO's window at E = 3940 (fixed poses on edges)."""
    G, _, t0, t1 = B.case(name)
    assert cb.plan_supported(G.E, t0, t1, 3)
    P, K, dX = _forward(cb, G, gpu, t0, t1, iters)
    _check(name, P, K, dX, iters, "window")


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("name", ["cfg1", "cfg2"])
def test_multikernel_gated(cb, gpu, multikernel, name, iters):
    """ba.hip (select_path(2)) on the cfg1 and cfg2 cases."""
    G, _, t0, t1 = B.case(name)
    P, K, dX = _forward(cb, G, gpu, t0, t1, iters)
    _check(name, P, K, dX, iters, "multikernel")


@pytest.mark.parametrize("iters", [1, 2])
def test_large_gated(cb, gpu, iters):
    """ba_large.hip: cfg4s, N = 95 free poses."""
    G, _, t0, t1 = B.case("cfg4s")
    assert t1 - t0 > 16 and not cb.plan_supported(G.E, t0, t1, 3)
    P, K, dX = _forward(cb, G, gpu, t0, t1, iters, eff=True)
    _check("cfg4s", P, K, dX, iters, "large")


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("path", [0, 2], ids=["window", "multikernel"])
def test_structure_only_gated(cb, gpu, path, iters):
    """t0 == t1 on the cfg1 case: dZ = Q u over the open edges and the clamps."""
    G, _, t0, t1 = B.case("struct")
    cb.select_path(path)
    try:
        P, K, dX = _forward(cb, G, gpu, t0, t1, iters)
    finally:
        cb.select_path(0)
    _check("struct", P, K, dX, iters, "structure " + ("multikernel" if path else "window"))


@pytest.mark.parametrize("name", ["cfg2", "dpvo10"])
def test_planned_and_fused_plans_are_bit_identical_gated(cb, gpu, name):
    """On gated graphs too, fastba.plan + BA(plan=ws) and the plan of the fused
    reproject(mem=, plan_window=) launch give BA()'s bits."""
    from dpvo_amd import fastba

    G, _, t0, t1 = B.case(name)
    D = G.to(gpu)
    lm = torch.tensor([B.LM], device=gpu)
    P0, K0 = D.poses.clone(), D.patches.clone()
    fastba.BA(P0, K0, D.intrinsics, D.target, D.weight, lm, D.ii, D.jj, D.kk, t0, t1, M=G.M,
              iterations=2)
    ws = fastba.plan(D.ii, D.jj, D.kk, t0, t1, D.patches.shape[0], D.poses.shape[0])
    assert ws is not None
    mem = int(D.jj.max().item()) + 1
    _, _, ws_fused = fastba.reproject(D.poses, D.patches, D.intrinsics, D.ii, D.jj, D.kk, mem=mem,
                                      plan_window=(t0, t1))
    for w in (ws, ws_fused):
        poses, patches = D.poses.clone(), D.patches.clone()
        fastba.BA(poses, patches, D.intrinsics, D.target, D.weight, lm, D.ii, D.jj, D.kk, t0, t1,
                  M=G.M, iterations=2, plan=w)
        assert torch.equal(poses, P0) and torch.equal(patches, K0)
    assert cb.check_status(D.poses) == 0
