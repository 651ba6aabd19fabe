"""The multi-kernel BA path's set-up (ba.hip ba_setup_kernel, select_path(2))
at the boundaries of its integer scans (ba_scan_cases.BA_SCAN_CASES): one edge,
a wave of patches (63 / 64 / 65), the workgroup (1023 / 1024 / 1025 edges), a
histogram of several scan chunks (33000 patch rows) and the bitonic fallback
(50000 rows).

The scans are integer, so they fix no summation order: every case must return
what the commit before the shared-scan change returned, bit for bit
(tests/golden/ba_scan_parent.npz, oracle/make_ba_scan_golden.py).  Spreading
the patch ids over a larger buffer does not change the mathematics, so the two
relabelled cases must also meet test_ba_gpu.test_ba_matches_oracle's bars for
cfg1 against the oracle."""
import functools

import numpy as np
import pytest
import torch

import oracle
from ba_scan_cases import BA_SCAN_CASES, ITERS, RELABELLED
from conftest import assert_ba_rel, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    m = dpvo_amd.load_extension("cuda_ba")
    m.check_status(torch.zeros(1, device=gpu))  # clean slate
    m.select_path(2)
    yield m
    m.select_path(0)


@pytest.fixture(scope="module")
def parent():
    return golden("ba_scan_parent")


@functools.lru_cache(maxsize=None)
def _run(cb, gpu, case):
    """(graph, t0, t1, poses, patches) of one BA call on the case, run once."""
    G, t0, t1, iters = BA_SCAN_CASES[case]()
    D = G.to(gpu)
    poses, patches = D.poses.clone(), D.patches.clone()
    cb.forward(poses, patches, D.intrinsics, D.target, D.weight, torch.tensor([1e-4], device=gpu),
               D.ii, D.jj, D.kk, G.M, t0, t1, iters, False)
    assert cb.check_status(poses) == 0
    return G, t0, t1, poses.cpu().numpy(), patches.cpu().numpy()


@pytest.mark.parametrize("case", list(BA_SCAN_CASES))
def test_matches_parent_bits(cb, gpu, parent, case):
    G, t0, t1, P, K = _run(cb, gpu, case)
    K0 = G.patches.numpy()
    touched = np.unique(G.kk.numpy())
    assert np.array_equal(P, parent[case + "__poses"])
    depth = parent[case + "__depth"]
    assert depth.shape == touched.shape
    # a touched patch holds its new inverse depth in every pixel
    assert np.array_equal(K[touched, 2], np.broadcast_to(depth[:, None, None], K[touched, 2].shape))
    rest = np.ones(K.shape[0], bool)
    rest[touched] = False
    assert np.array_equal(K[rest], K0[rest])
    assert np.array_equal(K[:, :2], K0[:, :2])  # x, y never change


@pytest.mark.parametrize("case", RELABELLED)
def test_relabelled_matches_oracle(cb, gpu, case):
    G, t0, t1, P, K = _run(cb, gpu, case)
    P0, K0 = G.poses.numpy(), G.patches.numpy()
    Pr, Kr = oracle.ba(P0, K0, G.intrinsics.numpy(), G.target.numpy(), G.weight.numpy(), 1e-4,
                       G.ii.numpy(), G.jj.numpy(), G.kk.numpy(), t0, t1, ITERS)
    # the bars of test_ba_gpu._check
    assert_ba_rel(P, K, Pr, Kr, P0, K0, t0, t1)
    np.testing.assert_allclose(P, Pr, rtol=0, atol=2e-5)
    np.testing.assert_allclose(K[:, 2], Kr[:, 2], rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(K[:, :2], Kr[:, :2])
