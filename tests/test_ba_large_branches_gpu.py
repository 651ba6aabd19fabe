"""Every band, border and status branch of the large-graph F-BA (ba_large.hip)
on graphs built to reach it (gba_cases.py; test_oracle_gba_cases.py proves on
the CPU that each graph has the structure its row claims), against the oracle
(dense fp64 S + Cholesky).

The solver is driven two ways: staged (gba_setup / gba_build / gba_packed /
gba_solve_update / gba_info), which also exposes the packed [y | S blocks]
system so that a wrong k_block and a wrong solver do not look the same, and
through cuda_ba.forward / forward_dx forced onto the large-graph path
(select_path(4)), which also gives the last iteration's dX.

Bars: packed S and y |got - ref| <= 1e-9 max|ref| (both sides sum the same
fp32 per-edge products in fp64, in a different order); parity exactly as
test_ba_large_gpu._check: delta ratios <= 1e-4 (conftest.assert_ba_rel), poses
2e-5 abs, inverse depths 1e-4 rel + 1e-5, patch x / y bit-equal.

Achieved on the MI355X (worst of the staged and the forward run and of 1 and 2
iterations; S and y as |got - ref| / max|ref|, bar 1e-9; dP / dZ / dX as
||got - ref|| / ||ref||, bar 1e-4; poses as max abs error, bar 2e-5; depth as
the largest error in units of its bar 1e-4 |ref| + 1e-5; 0 = bit-equal to
the oracle):

  case                          S        y       dP       dZ       dX    poses    depth
  chain_n1                2.3e-16  5.3e-17        0        0  3.8e-13        0        0
  chain_n2                5.3e-16  3.0e-16        0        0  1.1e-10        0        0
  chain_n3                3.7e-16  3.3e-16        0        0  9.2e-12        0        0
  chain_n4                4.0e-16  1.2e-15        0        0  5.2e-12        0        0
  chain_n5                4.1e-16  5.0e-16        0        0  5.4e-12        0        0
  chain_n6                3.1e-16  4.0e-16        0        0  1.2e-11        0        0
  chain_n7                2.8e-16  2.4e-16        0        0  1.1e-11        0        0
  chain_n9                4.7e-16  2.2e-16        0        0  2.2e-11        0        0
  g2                      3.7e-16  2.4e-16        0        0  9.6e-13        0        0
  g5_pad                  5.0e-16  3.1e-16        0        0  3.3e-13        0        0
  g13_pad                 6.6e-16  6.2e-16        0        0  1.6e-12        0        0
  g14_pad                 5.8e-16  2.7e-16        0        0  1.1e-12        0        0
  g16                     5.4e-16  4.1e-16        0        0  1.0e-12        0        0
  g16_pad                 3.4e-16  5.6e-16        0        0  1.6e-12        0        0
  g13_nsb6                5.3e-16  3.2e-16        0        0  1.1e-12        0        0
  g14_nsb6                1.0e-15  4.8e-16        0        0  1.6e-12        0        0
  g16_nsb4                5.3e-16  3.5e-16        0        0  1.8e-12        0        0
  nB1                     3.9e-16  3.4e-16        0        0  5.1e-13        0        0
  nB16                    7.2e-16  4.8e-16        0        0  1.4e-12        0        0
  nB17                    7.5e-16  4.6e-16        0        0  1.8e-12        0        0
  nB64                    8.9e-16  6.1e-16        0        0  1.4e-12        0        0
  border_then_interior    8.1e-16  3.8e-16        0        0  1.3e-12        0        0
  border_pair             5.5e-16  4.0e-16        0        0  2.0e-11        0        0
  border_many_sb          5.5e-16  2.9e-16        0        0  1.4e-11        0        0
  chain_like_nB17         6.8e-16  8.7e-16        0        0  7.5e-12        0        0
  set24                   4.9e-16  3.0e-16  4.0e-09        0  3.5e-11  5.8e-11        0
  isolated                2.6e-16  2.8e-16        0        0  2.2e-11        0        0
  duplicates              7.7e-16  4.1e-16        0        0  6.2e-13        0        0
  fixed_prefix            6.1e-16  3.8e-16        0        0  1.9e-12        0        0

Run with -s to print these figures.
"""
import numpy as np
import pytest
import torch

import gba_cases as gc
import oracle
from conftest import REL_TOL, assert_ba_rel, rel_err
from dpvo_amd import synthetic

pytestmark = pytest.mark.gpu

PACKED_TOL = 1e-9
_ref = {}


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    return dpvo_amd.load_extension("cuda_ba")


def _np(G):
    return (G.poses.numpy(), G.patches.numpy(), G.intrinsics.numpy(), G.target.numpy(),
            G.weight.numpy(), 1e-4, G.ii.numpy(), G.jj.numpy(), G.kk.numpy())


def _oracle(name, iters):
    """oracle.ba with diagnostics for a case of the table (computed once and
    shared; read-only)."""
    if (name, iters) not in _ref:
        G, t0 = gc.graph(name), gc.CASES[name]["t0"]
        _ref[name, iters] = oracle.ba(*_np(G), t0, G.F, iters, diagnostics=True)
    return _ref[name, iters]


def _lm(gpu):
    return torch.tensor([1e-4], device=gpu)


def _drain(cb, gpu):
    """Empty the device's sticky status accumulator (an earlier forward of
    any module may have left bits in it), so that what a test reads after its
    own call is that call's status whatever ran before."""
    try:
        cb.check_status(torch.zeros(1, device=gpu))
    except RuntimeError:
        pass


def _forward(cb, G, gpu, t0, iters):
    """cuda_ba.forward_dx on the large-graph path -> poses, patches, dX."""
    _drain(cb, gpu)
    D = G.to(gpu)
    poses, patches = D.poses.clone(), D.patches.clone()
    cb.select_path(4)
    try:
        dX = cb.forward_dx(poses, patches, D.intrinsics, D.target, D.weight, _lm(gpu), D.ii, D.jj,
                           D.kk, G.M, t0, G.F, iters, True)
        torch.cuda.synchronize()
    finally:
        cb.select_path(0)
    return poses.cpu().numpy(), patches.cpu().numpy(), dX.cpu().numpy()


def _setup(cb, G, gpu, t0):
    D = G.to(gpu)
    ws = cb.gba_setup(D.ii, D.jj, D.kk, D.patches.shape[0], G.M, t0, G.F, -(2**31) + 1,
                      2**31 - 1)
    return ws, D, cb.gba_info(ws, G.E, t0, G.F).cpu().tolist()


def _iterate(cb, ws, D, G, gpu, t0, poses, patches, weight=None):
    cb.gba_build(ws, poses, patches, D.intrinsics, D.target, D.weight if weight is None else weight,
                 _lm(gpu), D.ii, D.jj, t0, G.F)
    cb.gba_solve_update(ws, poses, patches, G.E, t0, G.F)


def _check(tag, P, K, Pr, Kr, G, t0, dX=None, dXr=None):
    """test_ba_large_gpu._check plus the dX ratio; prints what it measured."""
    P0, K0 = G.poses.numpy(), G.patches.numpy()
    e = {"dP": rel_err(P[t0:] - P0[t0:], Pr[t0:] - P0[t0:]),
         "dZ": rel_err(K[:, 2] - K0[:, 2], Kr[:, 2] - K0[:, 2])}
    if dX is not None:
        e["dX"] = rel_err(dX, dXr)
    e["pose_abs"] = float(np.abs(P - Pr).max())
    e["depth"] = float((np.abs(K[:, 2] - Kr[:, 2]) / (1e-4 * np.abs(Kr[:, 2]) + 1e-5)).max())
    print(f"\nRATIO {tag} " + " ".join(f"{k}={v:.3g}" for k, v in e.items()))
    assert_ba_rel(P, K, Pr, Kr, P0, K0, t0, G.F, dX, dXr, tol=REL_TOL)
    np.testing.assert_allclose(P, Pr, rtol=0, atol=2e-5)
    np.testing.assert_allclose(K[:, 2], Kr[:, 2], rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(K[:, :2], Kr[:, :2])
    np.testing.assert_array_equal(P[:t0], P0[:t0])  # fixed poses: bit-unchanged
    return e


def _dense_from_packed(packed, st, N):
    """The packed [y | lower S blocks in ascending lblk order] as (damped dense
    block-lower S, y, mask of the entries the packed system defines)."""
    y = packed[:6 * N]
    blk = packed[6 * N:].reshape(-1, 6, 6)
    assert blk.shape[0] == len(st["blocks"])
    keys = [gc.lblk(a, b) for a, b in st["blocks"]]
    assert keys == sorted(keys)
    S = np.zeros((N, 6, N, 6))
    mask = np.zeros((N, 6, N, 6), bool)
    for a in range(N):
        for b in range(a + 1):
            mask[a, :, b, :] = True  # a block the solver does not store is a zero block
    for (a, b), v in zip(st["blocks"], blk):
        S[a, :, b, :] = v
    S, mask = S.reshape(6 * N, 6 * N), mask.reshape(6 * N, 6 * N)
    d = np.arange(6 * N)
    S[d, d] += 1e-4 * S[d, d] + 1.0  # k_assemble / ba_cuda.cu:560; a bare pose keeps its 1
    return S, y, mask


@pytest.mark.parametrize("name", gc.PARITY)
def test_staged_structure_packed_system_and_parity(cb, gpu, name):
    """a. gba_info equals the restated structure; b. the packed system equals
    the oracle's damped S and y; c. one and two staged iterations match the
    oracle."""
    G, t0, st = gc.graph(name), gc.CASES[name]["t0"], gc.case_structure(name)
    N = G.F - t0
    ws, D, info = _setup(cb, G, gpu, t0)
    assert info == [0, st["nuniq"], st["nitems"], st["nblk"], st["nI"], st["nB"], st["g"],
                    st["nsb"]]
    assert tuple(info[4:]) == gc.CASES[name]["expect"]
    poses, patches = D.poses.clone(), D.patches.clone()
    cb.gba_build(ws, poses, patches, D.intrinsics, D.target, D.weight, _lm(gpu), D.ii, D.jj, t0,
                 G.F)
    packed = cb.gba_packed(ws, G.E, t0, G.F, st["nblk"]).cpu().numpy().copy()
    _, _, d1 = _oracle(name, 1)
    S, y, mask = _dense_from_packed(packed, st, N)
    rs = np.abs(S - d1["S"])[mask].max() / np.abs(d1["S"]).max()
    ry = np.abs(y - d1["y"]).max() / np.abs(d1["y"]).max()
    print(f"\nRATIO {name} packed S={rs / PACKED_TOL:.3g} y={ry / PACKED_TOL:.3g} "
          "(x 1e-9 max|ref|)")
    assert rs <= PACKED_TOL and ry <= PACKED_TOL, (rs, ry)
    cb.gba_solve_update(ws, poses, patches, G.E, t0, G.F)
    for iters in (1, 2):
        if iters == 2:
            _iterate(cb, ws, D, G, gpu, t0, poses, patches)
        torch.cuda.synchronize()
        Pr, Kr, _ = _oracle(name, iters)
        _check(f"{name} staged it{iters}", poses.cpu().numpy(), patches.cpu().numpy(), Pr, Kr, G,
               t0)
    assert cb.gba_info(ws, G.E, t0, G.F).cpu().tolist() == info  # status still 0


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("name", gc.PARITY)
def test_forward_on_large_path_matches_oracle(cb, gpu, name, iters):
    """c. cuda_ba.forward_dx forced onto the large-graph path: poses, depths
    and the last iteration's dX."""
    G, t0 = gc.graph(name), gc.CASES[name]["t0"]
    P, K, dX = _forward(cb, G, gpu, t0, iters)
    assert cb.check_status(torch.zeros(1, device=gpu)) == 0
    Pr, Kr, d = _oracle(name, iters)
    _check(f"{name} forward it{iters}", P, K, Pr, Kr, G, t0, dX, d["dX"])
    if name == "isolated":  # the free pose without any edge does not move
        f = gc.CASES[name]["args"]["extra"]["isolate"]
        np.testing.assert_array_equal(P[f], G.poses.numpy()[f])
        np.testing.assert_array_equal(Pr[f], G.poses.numpy()[f])
        assert not dX[f - t0].any()


def test_no_state_leaks_between_calls(cb, gpu):
    """d. nB = 17 (in-HBM border inverse), then a g = 1 chain with another
    border and the same E and N (so the same workspace size: the allocator
    hands the second and third call the block the call before dirtied), then
    the first again: the two runs of the first are bit-identical."""
    A, B = gc.graph("nB17"), gc.graph("chain_like_nB17")
    assert (A.E, A.F) == (B.E, B.F)
    a1 = _forward(cb, A, gpu, 1, 2)
    _forward(cb, B, gpu, 1, 2)
    a2 = _forward(cb, A, gpu, 1, 2)
    for x, y in zip(a1, a2):
        np.testing.assert_array_equal(x, y)
    assert cb.check_status(torch.zeros(1, device=gpu)) == 0


def test_too_many_border_poses_takes_no_pose_step(cb, gpu):
    """e. nB65: 65 border poses exceed kMaxBorder = 64.  From the code:
    k_structure sets kStBorder (8) and writes nsb = nB = 0, k_assemble and
    k_assemble_y return on the bit, k_final_dx writes dX = 0, and k_update
    retracts with the zero tangent (Exp(0) is the exact identity quaternion
    and zero translation in retrSE3, so poses are bit-unchanged) and steps the
    depths by dZ = Q u, the oracle's structure-only step."""
    name = "nB65"
    G, t0 = gc.graph(name), gc.CASES[name]["t0"]
    ws, D, info = _setup(cb, G, gpu, t0)
    assert info[0] & gc.ST_BORDER and info[7] == 0 and info[5] == 0
    poses, patches = D.poses.clone(), D.patches.clone()
    _iterate(cb, ws, D, G, gpu, t0, poses, patches)
    assert torch.equal(poses, D.poses)
    Pr, Kr = oracle.ba(*_np(G), t0, t0, 1)  # structure only: dZ = Q u
    K = patches.cpu().numpy()
    np.testing.assert_allclose(K[:, 2], Kr[:, 2], rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(K[:, :2], Kr[:, :2])
    assert np.abs(K[:, 2] - G.patches.numpy()[:, 2]).max() > 1e-5  # the depths did move
    P, K2, dX = _forward(cb, G, gpu, t0, 1)
    with pytest.raises(RuntimeError, match="status"):
        cb.check_status(torch.zeros(1, device=gpu))
    assert dX.shape == (G.F - t0, 6) and not dX.any()
    np.testing.assert_array_equal(P, G.poses.numpy())
    np.testing.assert_array_equal(K2, K)
    _forward(cb, gc.graph("nB64"), gpu, 1, 1)  # a following clean case reports 0
    assert cb.check_status(torch.zeros(1, device=gpu)) == 0


def test_patch_seen_from_25_free_poses_sets_status(cb, gpu):
    """e. set25: k_pset keeps the first kMaxSet = 24 poses it meets (ascending
    insertion, later ones dropped) and sets kStSet (4); the solve goes on with
    the truncated set, so the outputs are finite but not the reference's, and
    forward's status check raises.  set24 next to it is clean (parity cases)."""
    G = gc.graph("set25")
    ws, D, info = _setup(cb, G, gpu, 1)
    assert info[0] == gc.ST_SET
    P, K, dX = _forward(cb, G, gpu, 1, 2)
    with pytest.raises(RuntimeError, match="status"):
        cb.check_status(torch.zeros(1, device=gpu))
    assert np.isfinite(P).all() and np.isfinite(K).all() and np.isfinite(dX).all()
    assert _setup(cb, gc.graph("set24"), gpu, 1)[2][0] == 0


def test_patch_index_out_of_range_is_clamped(cb, gpu):
    """e. kk = num_patches and kk = -1: k_keys clamps the sort key to
    [0, num_patches) before anything indexes with it and sets kStClamp (2);
    k_lin reads patches through the clamped pkk.  The binding does not refuse
    such kk, so: status bit, finite outputs, and forward's status check
    raises."""
    src = gc.graph("g2")
    kk = src.kk.clone()
    kk[3], kk[7] = src.patches.shape[0], -1
    G = synthetic.Graph(src.poses, src.patches, src.intrinsics, src.ii, src.jj, kk, src.target,
                        src.weight, src.F, src.M)
    ws, D, info = _setup(cb, G, gpu, 1)
    assert info[0] == gc.ST_CLAMP
    assert info[1] == len(np.unique(np.clip(kk.numpy(), 0, src.patches.shape[0] - 1)))
    poses, patches = D.poses.clone(), D.patches.clone()
    _iterate(cb, ws, D, G, gpu, 1, poses, patches)
    torch.cuda.synchronize()
    assert torch.isfinite(poses).all() and torch.isfinite(patches).all()
    assert cb.gba_info(ws, G.E, 1, G.F).cpu().tolist()[0] == gc.ST_CLAMP
    P, K, dX = _forward(cb, G, gpu, 1, 1)
    with pytest.raises(RuntimeError, match="status"):
        cb.check_status(torch.zeros(1, device=gpu))
    assert np.isfinite(P).all() and np.isfinite(K).all() and np.isfinite(dX).all()


@pytest.mark.parametrize("name", ["border_then_interior", "nB17", "chain_n1"])
def test_failed_factorisation_gives_zero_step_and_clears(cb, gpu, name):
    """e. NaN weights: every pivot test `p > 0` fails (wg_bgj_inverse in
    k_cr_inv / k_border_solve, wg_gj_inverse for nB = 17), kStChol (1) is set,
    k_final_dx writes dX = 0 and the poses keep their bits.  The next
    gba_build clears the bit (k_clear_chol): with the clean weights the same
    workspace then gives the oracle's step."""
    G, t0 = gc.graph(name), gc.CASES[name]["t0"]
    ws, D, info = _setup(cb, G, gpu, t0)
    assert info[0] == 0
    nanw = torch.full_like(D.weight, float("nan"))
    poses, patches = D.poses.clone(), D.patches.clone()
    _iterate(cb, ws, D, G, gpu, t0, poses, patches, nanw)
    assert cb.gba_info(ws, G.E, t0, G.F).cpu().tolist()[0] == gc.ST_CHOL
    assert torch.equal(poses, D.poses)
    poses, patches = D.poses.clone(), D.patches.clone()
    _iterate(cb, ws, D, G, gpu, t0, poses, patches)
    torch.cuda.synchronize()
    assert cb.gba_info(ws, G.E, t0, G.F).cpu().tolist() == info
    Pr, Kr, _ = _oracle(name, 1)
    _check(f"{name} after NaN", poses.cpu().numpy(), patches.cpu().numpy(), Pr, Kr, G, t0)
    # the same through forward_dx: dX = 0, bit 1 reported but not fatal
    Dn = synthetic.Graph(G.poses, G.patches, G.intrinsics, G.ii, G.jj, G.kk, G.target,
                         torch.full_like(G.weight, float("nan")), G.F, G.M)
    P, _, dX = _forward(cb, Dn, gpu, t0, 1)
    assert cb.check_status(torch.zeros(1, device=gpu)) == gc.ST_CHOL
    assert not dX.any()
    np.testing.assert_array_equal(P, G.poses.numpy())
