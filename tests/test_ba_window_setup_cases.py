"""CPU checks of the case tables behind test_ba_window_setup_gpu.py: the host
restatement of the pose-slot function, and that every case reaches the branch
it is named for while the oracle stays off the depth clamps (a clamped depth
would hide a wrong set-up behind the clamp's constant)."""
import numpy as np
import pytest

import oracle
from ba_setup_cases import (BA_CASES, INT_MAX, K_HBM, PSLOT_CASES, fmin_of, patch_masks,
                            pslot_ref, wslot)


def test_wslot_restatement():
    # window [5, 9): N = 4 free poses, fixed poses from fmin = 2
    t0, N, fmin = 5, 4, 2
    assert wslot([5, 8], t0, N, fmin).tolist() == [0, 3]            # free poses
    assert wslot([2, 3, 4, 9], t0, N, fmin).tolist() == [4, 5, 6, 11]  # N + (gp - fmin)
    assert wslot([2 + 59, 2 + 60], t0, N, fmin).tolist() == [63, K_HBM]  # last slot, first past it
    assert wslot([1], t0, N, fmin).tolist() == [K_HBM]              # below fmin (cannot occur)
    assert wslot([0, 20], 0, 12, INT_MAX).tolist() == [0, K_HBM]    # no fixed pose
    # N = 0: the whole table holds fixed poses
    assert wslot([7, 7 + 63, 7 + 64], 3, 0, 7).tolist() == [0, 63, K_HBM]


def test_pslot_ref_orders_by_patch_then_edge():
    ii = np.array([0, 2, 1, 2], np.int64)
    jj = np.array([2, 1, 2, 0], np.int64)
    kk = np.array([9, 4, 9, 4], np.int64)
    ps, fmin = pslot_ref(ii, jj, kk, 1, 3, 3)  # free poses 1, 2; fixed pose 0 -> slot 2
    assert fmin == 0
    assert ps.tolist() == [1 | 0 << 8, 1 | 2 << 8, 2 | 1 << 8, 0 | 1 << 8]  # edges 1, 3, 0, 2


@pytest.mark.parametrize("case", list(PSLOT_CASES))
def test_pslot_case_reaches_its_branch(case):
    ii, jj, kk, M, F, (t0, t1) = PSLOT_CASES[case]()
    E, nk = kk.size, np.unique(kk).size
    assert 0 <= t0 and t1 <= F and t1 - t0 <= 16 and kk.max() < F * M
    ps, fmin = pslot_ref(ii, jj, kk, t0, t1, F)
    hbm = ((ps & 0xFF) == K_HBM) | ((ps >> 8) == K_HBM)
    if case == "E96_40patches":
        assert (E, nk) == (96, 40)
    if case == "E700_650patches":
        assert (E, nk) == (700, 650)
    if case == "E2048_1500patches_M2048":
        assert (E, nk, M) == (2048, 1500, 2048)
        assert kk.max() - kk.min() + 1 > 12288  # past the counting sort: bitonic path
    if case == "hbm_fixed_poses":
        assert hbm.any() and not hbm.all() and fmin + 64 - (t1 - t0) < t0
    else:
        assert not hbm.any() or fmin == INT_MAX
    if case == "no_fixed_pose":
        assert fmin == INT_MAX and fmin_of(ii, jj, t0, t1, F) == INT_MAX and not hbm.any()


@pytest.mark.parametrize("case", list(BA_CASES))
def test_ba_case_reaches_its_branch_off_the_clamps(case):
    G, t0, t1, iters = BA_CASES[case]()
    ii, jj, kk = G.ii.numpy(), G.jj.numpy(), G.kk.numpy()
    N, nuniq = t1 - t0, np.unique(kk).size
    masks = patch_masks(ii, jj, kk, t0, t1)
    ps, _ = pslot_ref(ii, jj, kk, t0, t1, G.poses.shape[0])
    hbm = ((ps & 0xFF) == K_HBM) | ((ps >> 8) == K_HBM)
    want_n = {"N0": 0, "N1": 1, "N2": 2, "N11": 11, "N16": 16}
    if case in want_n:
        assert N == want_n[case]
    if case == "no_free_pose_patches":
        assert (masks == 0).any() and (masks != 0).any()
    if case == "nuniq_gt_2048":
        assert nuniq > 2048
    if case in ("E2048", "E2049", "E8"):
        assert G.E == int(case[1:])
    if case == "hbm_fixed_poses":
        # an HBM-read fixed pose on an edge whose other end is free
        si, sj = ps & 0xFF, ps >> 8
        assert (((si == K_HBM) & (sj < N)) | ((sj == K_HBM) & (si < N))).any()
    else:
        assert not hbm.any()
    if case.startswith("dpvo"):
        assert G.F == 10 and iters == int(case[-1]) and G.E <= 10240
    # the oracle, iteration by iteration: no depth lands on a clamp (> 20 -> 1, < 1e-4 -> 1e-4)
    a = [x.numpy() for x in (G.poses, G.patches, G.intrinsics, G.target, G.weight)]
    touched = np.unique(kk)
    for it in range(1, iters + 1):
        Pr, Kr = oracle.ba(*a, 1e-4, ii, jj, kk, t0, t1, it)
        d = Kr[touched, 2, 0, 0]
        assert np.isfinite(Pr).all() and np.isfinite(d).all()
        assert (d > 2e-4).all() and (d < 20).all() and (d != 1.0).all(), (case, it, d.min(), d.max())
    moved = np.abs(Kr[touched, 2, 0, 0] - G.patches.numpy()[touched, 2, 0, 0]).max()
    assert moved > 1e-6  # the BA does something
