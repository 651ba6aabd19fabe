"""The window kernel's dense solve (ba_solve.hpp) at the window sizes where it
takes different paths after the factorisation: wave 3 converts block columns
to LDL^T form during the factor steps, and the columns it cannot take
(N - 11 of them: none up to N = 11, one at N = 12, five at N = 16, the largest
window) are converted by the whole workgroup afterwards.  Each size runs the
default F-BA path against the fp64 oracle with test_ba_gpu's bars (pose and
inverse-depth deltas 1e-4 relative, poses 2e-5 absolute, inverse depths 1e-4
relative + 1e-5)."""
import numpy as np
import pytest
import torch

import oracle
from conftest import assert_ba_rel
from dpvo_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    return dpvo_amd.load_extension("cuda_ba")


@pytest.mark.parametrize("N", [10, 11, 12, 13, 16])
def test_window_solve_leftover_columns(cb, gpu, N):
    F, M = N + 1, 48
    G = synthetic.make_graph(F=F, M=M, E=int(1.78 * F * M), seed=N)  # cfg2's edges per patch
    assert G.E <= 2048
    t0, t1, iters = 1, F, 2
    D = G.to(gpu)
    poses, patches = D.poses.clone(), D.patches.clone()
    cb.forward(poses, patches, D.intrinsics, D.target, D.weight,
               torch.tensor([1e-4], device=gpu), D.ii, D.jj, D.kk, G.M, t0, t1, iters, False)
    assert cb.check_status(poses) == 0
    P, K = poses.cpu().numpy(), patches.cpu().numpy()
    Pr, Kr = oracle.ba(G.poses.numpy(), G.patches.numpy(), G.intrinsics.numpy(),
                       G.target.numpy(), G.weight.numpy(), 1e-4, G.ii.numpy(), G.jj.numpy(),
                       G.kk.numpy(), t0, t1, iters)
    assert_ba_rel(P, K, Pr, Kr, G.poses.numpy(), G.patches.numpy(), t0, t1)
    np.testing.assert_allclose(P, Pr, rtol=0, atol=2e-5)
    np.testing.assert_allclose(K[:, 2], Kr[:, 2], rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(K[:, :2], Kr[:, :2])
