"""CPU: the gated BA cases of tests/ba_gates.py under the C oracle.

test_ba_gates_gpu.py holds the three HIP solvers to oracle.ba on these cases;
this file keeps that comparison from going vacuous and pins the oracle's own
gate.  The oracle runs one iteration at a time, and on the state entering
each of the two iterations every gate must close edges on its own, both
clamps of the retraction must fire, and no edge may sit next to a threshold
(the GPU's fp32 edge arithmetic and the oracle's must take the same branch).
The oracle's damped S and y are compared with ba_gates.normal_equations, an
fp64 numpy statement written from the formulas; both read the gate's
comparisons off ba_cuda.cu:296, 305-306 (Z >= 0.2 for rho, strict < 128,
strict > 0.2, strict bounds) and :218-221 (d > 20 -> 1, then max(d, 1e-4)).

measured (oracle vs restatement, ||.||_F relative, iteration 1 / 2):
  case     ungated S        gated S          ungated y        gated y          cond(S) gated
  cfg1     6.2e-8 / 8.8e-8  6.9e-8 / 2.8e-7  3.5e-6 / 2.7e-5  3.6e-6 / 2.2e-7  1.3e5 / 1.5e6
  cfg2     2.2e-8 / 2.5e-8  8.1e-8 / 4.8e-8  6.9e-6 / 9.3e-5  5.8e-6 / 1.0e-5  1.3e6 / 1.3e6
  n16      4.5e-8 / 4.2e-8  7.9e-8 / 8.0e-8  9.4e-6 / 4.9e-5  5.7e-6 / 1.4e-6  1.9e5 / 3.6e5
  dpvo10   2.9e-8 / 2.5e-8  4.3e-8 / 3.8e-8  1.2e-5 / 2.3e-4  9.7e-6 / 3.3e-5  2.2e2 / 2.2e2
  cfg4s    2.5e-7 / 5.5e-7  5.0e-7 / 9.6e-7  7.6e-6 / 1.1e-5  1.3e-5 / 2.5e-6  5.6e5 / 6.3e6
On the ungated graph only the fp32 rounding of the oracle's edge arithmetic
differs; the gated bar is 10 x that (the worst ratio above is 3.6).  y of the
second iteration is small against its terms, hence its larger relative error
on both graphs.  With the open edges at Z < 0.6 at full weight the gated S
error is 20 x the ungated one on cfg2 and dpvo10: the Jacobians grow as
1 / Z^2 with a Z formed by cancellation in fp32, and those few edges are most
of ||S||.  gate_graph therefore scales those edges' weights down, as it does
for the inverse-depth-20 patches; their closed edges keep the full weight.
Flipping the gate of one edge in the restatement moves S by 8e-4 .. 5e-1,
three decades above the bar.  Structure only: dZ = Q u within 8e-7."""
import numpy as np
import pytest

import ba_gates as B


@pytest.mark.parametrize("name", B.CASES)
def test_case_reaches_every_gate_and_clamp(name):
    """The section-2 conditions on the state entering each iteration."""
    G, info, t0, t1 = B.case(name)
    st = B.oracle_states(name)
    for it in (1, 2):
        f = B.conditions(G, t0, t1, st, it)
        print(name, "iteration", it, f)
        assert f["finite"] and f["status"] == 0           # oracle finite, Cholesky fine
        assert f["only_r"] >= 8                             # closed by |r| >= 128 alone
        assert f["only_z"] >= 8                             # closed by Z <= 0.2 alone
        assert f["only_b"] >= 8                             # closed by the bounds alone
        assert f["behind"] >= 8                             # depth-gated with Z < 0
        assert f["near128"] >= 8                            # 100 <= |r| < 128 and open
        assert f["wrap"] >= 3                               # d + dZ > 20 -> 1
        assert f["low"] >= 8                                # d + dZ < 1e-4 -> 1e-4
        assert f["margin"] >= 1e-3                          # relative distance to every threshold
        assert f["absz"] >= 1e-2
        assert f["dist20"] >= 1e-3                          # |d + dZ - 20|
        assert f["step"] <= 0.5                             # largest per-pose step
        assert B.conditions_hold(f)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "struct"])
def test_dead_structure(name):
    """The dead patch (every edge gated): C = 0, dZ = 0 exactly, its depth
    keeps its bits.  The dead pose: its S block is the damping alone (identity
    row and column), y and dX are 0.  Zero weights stay zero."""
    G, info, t0, t1 = B.case(name)
    st = B.oracle_states(name)
    kk = G.kk.numpy()
    kx = np.unique(kk)
    assert info["dead_patch"] is not None or info["dead_pose"] is not None
    for it in (1, 2):
        c = B.classify(G, st[it - 1][0], st[it - 1][1])
        d = st[it][2]
        k = info["dead_patch"]
        if k is not None:
            assert not c["open"][kk == k].any()
            assert d["dZ"][np.searchsorted(kx, k)] == 0.0
            np.testing.assert_array_equal(st[it][1][k], G.patches.numpy()[k])
        n = info["dead_pose"]
        if t1 > t0 and n is not None:
            assert not c["open"][(G.ii.numpy() == n) | (G.jj.numpy() == n)].any()
            b = slice(6 * (n - t0), 6 * (n - t0) + 6)
            for S in (d["S"], B.normal_equations(G, st[it - 1][0], st[it - 1][1], t0, t1)["S"]):
                np.testing.assert_array_equal(S[b, b], np.eye(6))
                assert not S[b, :6 * (n - t0)].any() and not S[b, 6 * (n - t0) + 6:].any()
            assert not d["y"][b].any() and not d["dX"][n - t0].any()
    assert (G.weight.numpy()[info["zero"]] == 0).all() and info["zero"].size >= 8


def _errors(G, st, t0, t1, it, **kw):
    ne = B.normal_equations(G, st[it - 1][0], st[it - 1][1], t0, t1, **kw)
    d = st[it][2]
    return B.mat_err(d["S"], ne["S"]), B.mat_err(d["y"], ne["y"]), ne


@pytest.mark.parametrize("name", [n for n in B.CASES if n != "struct"])
def test_oracle_gate_matches_restatement(name):
    """The oracle's damped S and y on the gated case against the fp64
    restatement, each within 10 x the same error on the ungated graph of the
    shape; flipping one edge's gate in the restatement moves S past that bar
    (one closed edge of each gate opened, one open edge closed, each with a
    free pose and weight >= 0.1)."""
    G, info, t0, t1 = B.case(name)
    st = B.oracle_states(name)
    U, u0, u1 = B.ungated(name)
    su = B.states_of(U, u0, u1)
    ii, jj, w = G.ii.numpy(), G.jj.numpy(), G.weight.numpy()
    usable = (((ii >= t0) & (ii < t1)) | ((jj >= t0) & (jj < t1))) & (w.min(1) >= 0.1)
    for it in (1, 2):
        bS, by, _ = _errors(U, su, u0, u1, it)
        eS, ey, ne = _errors(G, st, t0, t1, it)
        print(f"{name} iteration {it}: S {eS:.2e} (ungated {bS:.2e})  y {ey:.2e} (ungated {by:.2e})"
              f"  cond(S) {np.linalg.cond(ne['S']):.1e}")
        assert eS <= 10 * bS and ey <= 10 * by
        c = B.classify(G, st[it - 1][0], st[it - 1][1])
        moved = []
        for kind in ("only_r", "only_z", "only_b", "open"):
            e = np.nonzero(c[kind] & usable)[0]
            assert e.size, kind
            fS = B.mat_err(B.normal_equations(G, st[it - 1][0], st[it - 1][1], t0, t1,
                                              flip=int(e[0]))["S"], ne["S"])
            moved.append(fS)
            assert fS > 10 * bS, (kind, int(e[0]), fS)
        print(f"  one flipped edge moves S by {min(moved):.2e} .. {max(moved):.2e}")


def test_structure_only_matches_restatement():
    """t0 == t1: dZ = Q u of the gated edges, against the restatement, at the
    fp32 edge rounding (1e-5 of the largest step; measured 8e-7)."""
    G, info, t0, t1 = B.case("struct")
    st = B.oracle_states("struct")
    for it in (1, 2):
        ne = B.normal_equations(G, st[it - 1][0], st[it - 1][1], t0, t1)
        dZ = ne["Q"] * ne["u"]
        err = np.abs(st[it][2]["dZ"] - dZ).max() / np.abs(dZ).max()
        print("struct iteration", it, "dZ error", err)
        assert err <= 1e-5


def test_assert_per_pose_sees_one_bad_pose():
    """A pose with a small step that is 1 % wrong passes the norm-wise bar and
    fails the per-pose one; the dead pose (reference step 0) is held to the
    floor ||dXr|| / sqrt(N)."""
    rng = np.random.default_rng(0)
    ref = rng.standard_normal((10, 6))
    ref[3] *= 1e-3
    ref[7] = 0
    got = ref.copy()
    assert B.assert_per_pose(got, ref) == 0.0
    got[3] *= 1.01
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-5
    B.assert_per_pose(got, ref)  # 1 % of a tiny step: inside the floor
    got[3] = ref[3] + 2e-4 * np.linalg.norm(ref) / np.sqrt(10) / np.sqrt(6)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-4
    with pytest.raises(AssertionError, match="pose 3"):
        B.assert_per_pose(got, ref)
    got = ref.copy()
    got[7] = 2e-4 * np.linalg.norm(ref) / np.sqrt(10) / np.sqrt(6)
    with pytest.raises(AssertionError, match="pose 7"):
        B.assert_per_pose(got, ref)
