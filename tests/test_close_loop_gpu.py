"""loop_closure.close_loop and loop_closure.apply_result on the device against
fp64 restatements: the RANSAC-Umeyama measurement (tests/umeyama_restatement.py),
the pose-graph LM (ref_run_pgo of tests/test_pgo_loop_gpu.py) and, for
apply_result, a numpy restatement of long_term.py:175-203 followed by
PatchGraph.normalize (patchgraph.py:93-106).

Measured on an MI355X: the estimate (121 inliers of 200 points, hypothesis 2,
s = 1.2998) within 8e-16 of the restatement; run_pgo's result against the fp64
restatement LM (30 iterations, 9.59e-3 -> 1.47e-3) differs by 4.9e-6 in
translation, 1.5e-7 in the quaternion, 4.1e-7 in scale (bounds 1e-4 / 1e-4 /
1e-5); apply_result 2.2e-7 (poses), 3.5e-8 (depths), 3.0e-8 (deltas) relative
(bound 1e-5).
"""
import numpy as np
import pytest
import torch

import sim3_restatement as R
import umeyama_restatement as U
from test_pgo_loop_gpu import make_loop, ref_run_pgo

F64 = torch.float64
N_FRAMES, I, J = 40, 38, 1


@pytest.fixture(scope="module")
def lc(gpu):
    from dpvo_amd import loop_closure

    return loop_closure


def make_clouds(Ti, Tij, N, seed, drift=1.3, noise=0.01, outlier_frac=0.4, H=400):
    """N world points seen from frame i (world-to-camera Ti) and from frame j
    = Tij Ti; frame j's cloud is scaled by `drift`, noisy, and a fraction of
    its rows are outliers.  Returns (i_pts, j_pts, samples [H, 3])."""
    g = np.random.default_rng(seed)
    cam = g.uniform(-2, 2, (N, 3))
    cam[:, 2] = g.uniform(1, 8, N)
    world = (cam - Ti[:3, 3]) @ Ti[:3, :3]            # Ti^-1 cam
    i_pts = world @ Ti[:3, :3].T + Ti[:3, 3]
    Tj = Tij @ Ti
    j_pts = drift * (world @ Tj[:3, :3].T + Tj[:3, 3]) + noise * g.standard_normal((N, 3))
    out = g.random(N) < outlier_frac
    j_pts[out] = g.uniform(-10, 10, (int(out.sum()), 3))
    samples = np.stack([g.choice(N, 3, replace=False) for _ in range(H)])
    return i_pts, j_pts, samples


@pytest.fixture(scope="module")
def loop():
    """The map (f32 world-to-camera poses of a drifted loop with one loop
    already closed), the matched clouds of a new pair, and the restatements'
    results on exactly those values."""
    c2w, dS, ii, jj = make_loop(N_FRAMES, 2)           # ii = [37, 38], jj = [0, 1]
    poses32 = R.to_data(R.inv(R.from_data(c2w)))[:, :7].float()
    W = R.from_data(poses32.double())                   # what the device holds, in fp64
    rigid = R.from_data(dS[1]).numpy().copy()           # a rigid motion between frames i and j
    rigid[:3, :3] /= np.cbrt(np.linalg.det(rigid[:3, :3]))
    i_pts, j_pts, samples = make_clouds(W[I].numpy(), rigid, 200, seed=21)
    est = U.ransac_umeyama(i_pts, j_pts, samples)
    assert est["status"] == 0 and est["num_inliers"] >= 100 and est["min_margin"] >= 1e-9
    assert abs(est["s"] - 1.3) < 1e-2
    new = torch.from_numpy(np.concatenate([est["t"], U.quaternion_of(est["R"]), [est["s"]]]))
    prev = R.to_data(W[0:1] @ R.inv(W[37:38]))          # G_j G_i^-1 of the earlier loop, scale 1
    loop_ii, loop_jj = torch.tensor([37, I]), torch.tensor([0, J])
    final, _, hist = ref_run_pgo(R.to_data(R.inv(W))[:, :7], torch.cat([prev, new[None]]),
                                 loop_ii, loop_jj)
    return dict(poses=poses32, i_pts=i_pts, j_pts=j_pts, samples=samples, est=est, final=final,
                hist=hist)


def _call(lc, gpu, loop, i_pts, j_pts, samples, **kw):
    poses_ = torch.zeros(48, 7)
    poses_[:, 6] = 1
    poses_[:N_FRAMES] = loop["poses"]
    poses_ = poses_.to(gpu)
    before = poses_.clone()
    out = lc.close_loop(poses_, N_FRAMES, torch.tensor([37], device=gpu),
                        torch.tensor([0], device=gpu), I, J, torch.from_numpy(i_pts).to(gpu),
                        torch.from_numpy(j_pts).to(gpu),
                        samples=torch.from_numpy(samples).to(gpu), **kw)
    assert torch.equal(poses_, before)  # the map is only read
    return out


@pytest.mark.gpu
def test_close_loop_matches_restatements(lc, gpu, loop):
    ref = loop["est"]
    final, loop_ii, loop_jj, est = _call(lc, gpu, loop, loop["i_pts"], loop["j_pts"],
                                         loop["samples"])
    assert loop_ii.tolist() == [37, I] and loop_jj.tolist() == [0, J]
    assert est.info.tolist() == [ref["num_inliers"], ref["winner"], ref["stop"], 0]
    assert np.array_equal(est.mask.cpu().numpy(), ref["mask"])
    err = max(np.abs(est.R.cpu().numpy() - ref["R"]).max(),
              np.abs(est.t.cpu().numpy() - ref["t"]).max(), abs(float(est.s) - ref["s"]))
    print("estimate: inliers", ref["num_inliers"], "hypothesis", ref["winner"], "s", ref["s"],
          "max abs error of R / t / s", err)
    assert est.R.dtype == torch.float64 and err <= 1e-10

    s = I + 1
    assert final.shape == (s, 8) and final.dtype == torch.float32
    got, want = final.double().cpu(), R.to_data(loop["final"])
    dt = (got[:, :3] - want[:, :3]).abs().max().item()
    dq = torch.minimum((got[:, 3:7] - want[:, 3:7]).abs().amax(1),
                       (got[:, 3:7] + want[:, 3:7]).abs().amax(1)).max().item()
    dsc = (got[:, 7] - want[:, 7]).abs().max().item()
    print(f"final: restatement LM {loop['hist'][0]:.3e} -> {loop['hist'][-1]:.3e} in "
          f"{len(loop['hist'])} iterations; max diff translation {dt:.3e} quaternion {dq:.3e} "
          f"scale {dsc:.3e}; scales {got[:, 7].min().item():.4f} .. {got[:, 7].max().item():.4f}")
    # the bound of test_run_pgo_end_to_end (device f32 LM against the fp64 restatement LM)
    assert dt <= 1e-4 and dq <= 1e-4 and dsc <= 1e-5


@pytest.mark.gpu
def test_close_loop_declines(lc, gpu, loop):
    i_pts, j_pts, samples = loop["i_pts"], loop["j_pts"], loop["samples"]
    # 9 points: numel 27 < 30
    assert _call(lc, gpu, loop, i_pts[:9], j_pts[:9], samples % 9) is None
    # the best count is below min_inliers
    few = U.ransac_umeyama(i_pts[:30], j_pts[:30], samples % 30)
    assert few["status"] == 0 and 0 < few["num_inliers"] < 30 and few["min_margin"] >= 1e-9
    assert _call(lc, gpu, loop, i_pts[:30], j_pts[:30], samples % 30) is None
    best = loop["est"]["num_inliers"]
    assert _call(lc, gpu, loop, i_pts, j_pts, samples, min_inliers=best + 1) is None
    # status 1: every sample is collinear (along an axis: exactly rank 1)
    line = np.outer(np.arange(40.0), [0.5, 0.0, 0.0])
    assert U.ransac_umeyama(line, line, samples % 40)["status"] == 1
    assert _call(lc, gpu, loop, line, line, samples % 40) is None


# ------------------------------------------------------------ apply_result
def ref_apply_result(final, poses, patches, n, M, log, pairs, count, tstamps):
    """long_term.py:175-203 and patchgraph.py:93-106 in fp64 numpy / 4x4
    matrices.  Returns (poses as 4x4 [N], patches, log)."""
    safe_i = final.shape[0]
    T = R.from_data(torch.from_numpy(poses)).numpy().copy()
    K = patches.reshape(-1, M, *patches.shape[1:]).copy()
    log = log.copy()
    s1 = np.ones(n)
    s1[:safe_i] = final[:, 7]
    T[:safe_i] = np.linalg.inv(R.from_data(torch.from_numpy(final[:, :7])).numpy())
    K[:safe_i, :, 2] /= final[:, 7].reshape(-1, 1, 1, 1)
    scale_of = {int(tstamps[k]): s1[k] for k in range(n)}
    delta = {int(pairs[r, 0]): int(pairs[r, 1]) for r in range(count)}
    for r in range(count):
        t_src = int(pairs[r, 0])
        while t_src in delta:
            t_src = delta[t_src]
        log[r, :3] *= scale_of[t_src]
    s = K[:n, :, 2].mean()
    K[:n, :, 2] /= s
    T[:n, :3, 3] *= s
    log[:, :3] *= s
    T[:n] = T[:n] @ np.linalg.inv(T[0])
    return T, K.reshape(patches.shape), log


def _rel(got, want):
    return float(np.linalg.norm(np.asarray(got, np.float64) - want) / np.linalg.norm(want))


@pytest.mark.gpu
def test_apply_result(lc, gpu):
    n, M, P, safe_i, cap, count = 12, 4, 3, 8, 8, 4
    g = torch.Generator().manual_seed(4)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=F64)  # noqa: E731

    def random_se3(k, spread):
        q = rnd(k, 4)
        q = q / q.norm(dim=1, keepdim=True)
        return torch.cat([spread * rnd(k, 3), q * torch.sign(q[:, 3:])], 1)

    poses = random_se3(16, 10.0).float()
    patches = torch.rand(16 * M, 3, P, P, generator=g) + 0.5
    final = torch.cat([random_se3(safe_i, 10.0),
                       torch.linspace(0.8, 1.3, safe_i, dtype=F64)[:, None]], 1).float()
    tstamps = torch.tensor([0, 2, 4, 5, 8, 10, 12, 14, 16, 18, 20, 22, 23, 24, 25, 26])
    # removed frames 3, 6, 7, 21: 3 -> keyframe 2 (index 1); 7 -> 6 -> keyframe 5
    # (index 3; 6 is itself removed: a chain of two records); 6 -> keyframe 5;
    # 21 -> keyframe 20 (index 10 >= safe_i: scale 1)
    pairs = torch.zeros(cap, 2, dtype=torch.long)
    pairs[:count] = torch.tensor([[3, 2], [7, 6], [6, 5], [21, 20]])
    pairs[count:] = torch.tensor([99, 98])  # stale rows beyond count are never followed
    log = random_se3(cap, 1.0).float()

    T, K, L = ref_apply_result(final.double().numpy(), poses.double().numpy(),
                               patches.double().numpy(), n, M, log.double().numpy(),
                               pairs.numpy(), count, tstamps.numpy())

    dp, dk, dl = poses.to(gpu), patches.to(gpu), log.to(gpu)
    delta = (dl, pairs.to(gpu), torch.tensor([count], dtype=torch.int32, device=gpu))
    s = lc.apply_result(final.to(gpu), dp, dk, n, M, delta=delta, tstamps=tstamps.to(gpu))
    want_s = patches.double().view(16, M, 3, P, P)[:n, :, 2].clone()
    want_s[:safe_i] /= final[:, 7].double().view(-1, 1, 1, 1)
    assert abs(float(s) - float(want_s.mean())) <= 1e-5 * float(want_s.mean())

    got_T = R.from_data(dp.double().cpu()).numpy()
    e_pose = _rel(got_T[:n], T[:n])
    e_depth = _rel(dk.cpu().numpy()[: n * M, 2], K[: n * M, 2])
    e_delta = _rel(dl.cpu().numpy()[:, :3], L[:, :3])
    print("apply_result relative errors: poses", e_pose, "depths", e_depth, "deltas", e_delta)
    assert e_pose <= 1e-5 and e_depth <= 1e-5 and e_delta <= 1e-5
    # per record: the scale its source keyframe carries
    ratio = (dl[:count, :3].double().cpu() / log[:count, :3].double()).mean(1) / float(s)
    want_ratio = torch.tensor([final[1, 7], final[3, 7], final[3, 7], 1.0], dtype=F64)
    assert torch.allclose(ratio, want_ratio, rtol=1e-5)
    # untouched: frames >= n, the patch coordinates, the rotations of the log
    assert torch.equal(dp[n:].cpu(), poses[n:])
    assert torch.equal(dk[n * M:].cpu(), patches[n * M:])
    assert torch.equal(dk[:, :2].cpu(), patches[:, :2])
    assert torch.equal(dl[:, 3:].cpu(), log[:, 3:])
    # frames in [safe_i, n) and the log's rows beyond count: normalize alone
    assert torch.allclose(dk[safe_i * M:n * M, 2].cpu() * s.cpu(), patches[safe_i * M:n * M, 2],
                          rtol=1e-6)
    assert torch.allclose(dl[count:, :3].cpu(), log[count:, :3] * s.cpu(), rtol=1e-6)

    # without a delta log; and a record that leads to no keyframe is an error
    dp2, dk2 = poses.to(gpu), patches.to(gpu)
    lc.apply_result(final.to(gpu), dp2, dk2, n, M)
    assert torch.equal(dp2, dp) and torch.equal(dk2, dk)
    bad = pairs.clone()
    bad[0, 1] = 1  # frame 1 is neither a keyframe nor a record
    with pytest.raises(ValueError, match="apply_result"):
        lc.apply_result(final.to(gpu), poses.to(gpu), patches.to(gpu), n, M,
                        delta=(log.to(gpu), bad.to(gpu), delta[2]), tstamps=tstamps.to(gpu))
