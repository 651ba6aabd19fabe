"""CPU: pins tests/frontend_ref.py (the oracle of test_frontend_gpu.py) by
properties -- the reference's lietorch cannot run without its CUDA backend."""
import numpy as np
import pytest
import torch

import frontend_ref as F
import se3_restatement as R


def _pose(rng, rot=0.3, trans=1.0):
    xi = np.concatenate([trans * rng.normal(size=3), rot * rng.normal(size=3)])
    return R.to_data(R.Exp(torch.as_tensor(xi))).numpy()


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    if np.dot(a[3:], b[3:]) < 0:
        b = np.concatenate([b[:3], -b[3:]])
    np.testing.assert_allclose(a, b, rtol=0, atol=tol)


def test_constant_velocity_is_P1_P2inv_P1():
    rng = np.random.default_rng(0)
    P1, P2 = _pose(rng), _pose(rng)
    A, B = R.from_data(torch.as_tensor(P1)), R.from_data(torch.as_tensor(P2))
    _close(F.motion_model(P1, P2, 1.0, 1.0), R.to_data(A @ R.inv(B) @ A).numpy())


def test_equal_poses_and_zero_damping_give_P1():
    rng = np.random.default_rng(1)
    P1, P2 = _pose(rng), _pose(rng)
    _close(F.motion_model(P1, P1, 3.0, 0.5), P1)
    _close(F.motion_model(P1, P2, 3.0, 0.0), P1)


@pytest.mark.parametrize("fac", [0.5, 1.0, 3.0])
def test_fac_scales_log_linearly(fac):
    rng = np.random.default_rng(2)
    P1, P2 = _pose(rng, rot=0.1), _pose(rng, rot=0.1)
    A, B = R.from_data(torch.as_tensor(P1)), R.from_data(torch.as_tensor(P2))
    xi = R.Log(A @ R.inv(B))
    got = R.from_data(torch.as_tensor(F.motion_model(P1, P2, fac, 0.5)))
    np.testing.assert_allclose(R.Log(got @ R.inv(A)).numpy(), (0.5 * fac * xi).numpy(), rtol=0,
                               atol=1e-12)


def test_time_factor():
    assert F.time_factor([0.0, 1.0, 3.0], 2) == 2.0
    assert F.time_factor([0.0, 1.0, 1.5, 9.0], 2) == 0.5  # later entries are not read
    assert F.time_factor([2.0, 2.0, 5.0], 2) == 1.0  # b == a
    assert F.time_factor([3.0, 4.0], 1) == 1.0 / 2.0  # a = 1 (the [1] * 3 padding)


@pytest.mark.parametrize("n", [1, 2, 3, 54, 189])
def test_lower_median_is_torch_median(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=n).astype(np.float32)
    assert F.lower_median(x) == torch.median(torch.from_numpy(x)).item()
    ties = rng.integers(0, 3, size=n).astype(np.float32)
    assert F.lower_median(ties) == torch.median(torch.from_numpy(ties)).item()


def test_lower_median_nan():
    x = np.array([1.0, np.nan, 3.0], np.float32)
    assert np.isnan(F.lower_median(x)) and torch.isnan(torch.median(torch.from_numpy(x)))


def test_identity_chain_returns_root_pose():
    rng = np.random.default_rng(3)
    poses = np.stack([_pose(rng), _pose(rng)])
    tstamps = np.array([0, 5])
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    rec = [(t, t - 1, ident) for t in (1, 2, 3, 4)]
    traj, root, info = F.trajectory(poses, tstamps, 2, rec, 6, inverse=False)
    for t in range(5):
        _close(traj[t], poses[0])
    _close(traj[5], poses[1])
    assert root.tolist() == [0, 0, 0, 0, 0, 1] and info.tolist() == [0, 0]


def test_trajectory_rules():
    rng = np.random.default_rng(4)
    poses = np.stack([_pose(rng), _pose(rng)])
    tstamps = np.array([0, 2])
    d1, d2, d3 = _pose(rng), _pose(rng), _pose(rng)
    # two records for t1 = 1 (the last wins), one for keyframe 2 (the keyframe
    # wins), one with t0 >= t1, one out of range, 3 -> 1 -> 0; frame 4 has no
    # record and 5 hangs on 4: both unresolved
    rec = [(1, 0, d1), (1, 0, d2), (2, 0, d3), (3, 3, d1), (9, 0, d1), (3, 1, d3), (5, 4, d1)]
    traj, root, info = F.trajectory(poses, tstamps, 2, rec, 6, inverse=False)
    M = lambda d: R.from_data(torch.as_tensor(d))  # noqa: E731
    _close(traj[1], R.to_data(M(d2) @ M(poses[0])).numpy())
    _close(traj[2], poses[1])
    _close(traj[3], R.to_data(M(d3) @ M(d2) @ M(poses[0])).numpy())
    assert np.isnan(traj[4]).all() and np.isnan(traj[5]).all()
    assert root.tolist() == [0, 0, 1, 0, -1, -1] and info.tolist() == [2, 2]
    inv, _, _ = F.trajectory(poses, tstamps, 2, rec, 6, inverse=True)
    np.testing.assert_allclose((M(inv[3]) @ M(traj[3])).numpy(), np.eye(4), atol=1e-12)


def test_init_frame_restatement_rows():
    rng = np.random.default_rng(5)
    N, M, P, n, counter = 6, 4, 3, 3, 7
    poses = np.stack([_pose(rng) for _ in range(N)]).astype(np.float32)
    patches = rng.uniform(0.1, 2.0, size=(N * M, 3, P, P)).astype(np.float32)
    intr = rng.uniform(1, 300, size=(N, 4)).astype(np.float32)
    ts = np.arange(N, dtype=np.int64)
    times = np.arange(10, dtype=np.float64)
    new = rng.uniform(size=(M, 3, P, P)).astype(np.float32)
    ni = np.array([320.0, 321.0, 160.5, 120.25], np.float32)
    p, k, i, t = F.init_frame(poses, patches, intr, ts, times, new, ni, n, counter, M, res=4.0)
    assert t[n] == counter and (i[n] == ni / np.float32(4)).all()
    s = torch.median(torch.from_numpy(patches[0:n * M, 2])).item()
    assert (k[n * M:(n + 1) * M, 2] == s).all()
    assert (k[n * M:(n + 1) * M, :2] == new[:, :2]).all()
    assert (k[:n * M] == patches[:n * M]).all() and (k[(n + 1) * M:] == patches[(n + 1) * M:]).all()
    _close(p[n], F.motion_model(poses[n - 1], poses[n - 2], 1.0, 0.5))
