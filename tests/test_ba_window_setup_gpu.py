"""The BA window kernel's set-up (ba_window.hip): the pose-slot pairs the plan
stores per sorted position, and the BA built on them.

pslot: exact equality with a host restatement (ba_setup_cases.pslot_ref),
through fastba.plan and through the fused reprojection launch, on repeated
calls; one call with t0 as a device scalar.

BA: every case of ba_setup_cases.BA_CASES against the oracle at the existing
bars (conftest.assert_ba_rel) with the status checked after every call, and
bit for bit (np.array_equal) against what the commit before the set-up change
returned (tests/golden/ba_setup_parent.npz, scripts/make_ba_setup_golden.py):
the set-up may only change how the lists are found, never the lists or a
summation order."""
import numpy as np
import pytest
import torch

import oracle
from ba_setup_cases import BA_CASES, META_BYTES, PSLOT_CASES, PSLOT_DEVICE_T0, pslot_ref
from conftest import assert_ba_rel, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    m = dpvo_amd.load_extension("cuda_ba")
    m.check_status(torch.zeros(1, device=gpu))  # clean slate
    return m


@pytest.fixture(scope="module")
def parent():
    return golden("ba_setup_parent")


def _pslot(cb, ws, E, t0, t1):
    off = cb.plan_offsets(E, t0, t1)
    b = ws.cpu().numpy()
    meta = np.frombuffer(b[off[4]:off[4] + 16].tobytes(), np.int32)
    at = off[4] + META_BYTES  # right behind the five pinned plan arrays
    return np.frombuffer(b[at:at + 2 * E].tobytes(), np.uint16), int(meta[1])


@pytest.mark.parametrize("case", list(PSLOT_CASES))
def test_pslot_matches_host_restatement(cb, gpu, case):
    from dpvo_amd import fastba

    ii, jj, kk, M, F, (t0, t1) = PSLOT_CASES[case]()
    E = kk.size
    want, fmin = pslot_ref(ii, jj, kk, t0, t1, F)
    D = [torch.from_numpy(x).to(gpu) for x in (ii, jj, kk)]
    for rep in range(2):
        ws = fastba.plan(*D, t0, t1, F * M, F)
        assert ws is not None
        got, f = _pslot(cb, ws, E, t0, t1)
        assert f == fmin
        np.testing.assert_array_equal(got, want)
    poses = torch.zeros(F, 7, device=gpu)
    poses[:, 6] = 1
    patches = torch.ones(F * M, 3, 3, 3, device=gpu)
    intr = torch.tensor([[80.0, 80.0, 80.0, 60.0]], device=gpu).repeat(F, 1)
    for rep in range(2):
        _, _, ws = fastba.reproject(poses, patches, intr, *D, mem=F, plan_window=(t0, t1))
        got, f = _pslot(cb, ws, E, t0, t1)
        assert f == fmin
        np.testing.assert_array_equal(got, want)
    if case == PSLOT_DEVICE_T0:
        t0d = torch.tensor([t0], dtype=torch.int32, device=gpu)
        _, _, ws = fastba.reproject_window_dev(poses, patches, intr, *D, F, t0d, t1 - t0)
        got, f = _pslot(cb, ws, E, t0, t1)
        assert f == fmin
        np.testing.assert_array_equal(got, want)
    assert cb.check_status(poses) == 0


@pytest.mark.parametrize("case", list(BA_CASES))
def test_ba_matches_oracle_and_parent_bits(cb, gpu, parent, case):
    G, t0, t1, iters = BA_CASES[case]()
    D = G.to(gpu)
    lm = torch.tensor([1e-4], device=gpu)
    outs = []
    for rep in range(2):
        poses, patches = D.poses.clone(), D.patches.clone()
        cb.forward(poses, patches, D.intrinsics, D.target, D.weight, lm, D.ii, D.jj, D.kk, G.M, t0,
                   t1, iters, False)
        assert cb.check_status(poses) == 0
        outs.append((poses.cpu().numpy(), patches.cpu().numpy()))
    P, K = outs[0]
    assert np.array_equal(P, outs[1][0]) and np.array_equal(K, outs[1][1])
    P0, K0 = G.poses.numpy(), G.patches.numpy()
    Pr, Kr = oracle.ba(P0, K0, G.intrinsics.numpy(), G.target.numpy(), G.weight.numpy(), 1e-4,
                       G.ii.numpy(), G.jj.numpy(), G.kk.numpy(), t0, t1, iters)
    if t1 > t0:
        assert_ba_rel(P, K, Pr, Kr, P0, K0, t0, t1)
    else:  # structure only: no pose moves, the inverse depths do
        from conftest import REL_TOL, rel_err

        assert np.array_equal(P, P0)
        assert rel_err(K[:, 2] - K0[:, 2], Kr[:, 2] - K0[:, 2]) <= REL_TOL
    assert np.array_equal(P[:t0], P0[:t0]) and np.array_equal(P[t1:], P0[t1:])  # fixed poses
    assert np.array_equal(P, parent[case + "__poses"])
    assert np.array_equal(K, parent[case + "__patches"])
