"""GPU: the long-term loop closure inside the tracker (dpvo_amd/long_term.py and
the four hooks of dpvo_amd/dpvo.py), on the stand-in network of
tests/test_tracker_gpu.py: a circle of LAP frames in x / z that returns to its
start, run for two laps and a few frames.

The detector projects fixed world landmarks through the truth pose of the
frame's timestamp (every pixel of the stand-in image is the timestamp), with
fixed {-1, 0, 1} / 8 descriptors, D = 32.  The scripted scorer answers, from
the second lap on, the first-lap keyframe nearest in truth pose."""
import numpy as np
import pytest
import torch

from test_tracker_gpu import HT, K_IMAGE, WD, StandIn, _cfg, _image, _K, _scaled_error

pytestmark = pytest.mark.gpu

LAP = 30
FRAMES = 2 * LAP + 8
# KEYFRAME_INDEX 2 with KEYFRAME_THRESH 1 px keeps the frames of this scene (as in
# test_tracker_gpu.test_loop_closure_wiring).  OPTIMIZATION_WINDOW 8 frees poses 1..7 in the
# twelve updates at n == 8: with _cfg's window of 4 only poses 4..7 move and the first frames
# never reach the truth (test_tracker_gpu.test_standin_scene_bookkeeping_and_accuracy says
# why), and the first loop of the second lap closes onto exactly those frames.  The default
# index with the same threshold drops two frames in three, which is what the cache test wants.
KEEP = dict(KEYFRAME_INDEX=2, KEYFRAME_THRESH=1.0, OPTIMIZATION_WINDOW=8, PATCH_LIFETIME=6,
            REMOVAL_WINDOW=10, MAX_EDGES=8000)
DROP = dict(KEYFRAME_THRESH=1.0)
NUM_LANDMARKS, D = 450, 32


class Detector:
    def __init__(self, net, dev):
        g = torch.Generator().manual_seed(21)
        z = torch.rand(NUM_LANDMARKS, generator=g) * 1.2 + 1.0
        x = (torch.rand(NUM_LANDMARKS, generator=g) - 0.5) * 1.5
        y = (torch.rand(NUM_LANDMARKS, generator=g) - 0.5) * 0.18 * z
        self.world = torch.stack([x, y, z], 1).to(dev)
        self.desc = (torch.randint(-1, 2, (NUM_LANDMARKS, D), generator=g).float() / 8).to(dev)
        self.net = net
        self.K = torch.tensor(K_IMAGE, device=dev)
        self.seen = []

    def camera(self, t):
        """The landmarks in the camera of timestamp t (the truth has no rotation)."""
        return self.world + self.net.gt_poses_t[t, :3]

    def visible(self, t):
        X = self.camera(t)
        fx, fy, cx, cy = self.K
        uv = torch.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
        ok = (uv[:, 0] > 2) & (uv[:, 0] < WD - 2) & (uv[:, 1] > 2) & (uv[:, 1] < HT - 2)
        return torch.nonzero(ok)[:, 0], uv

    def __call__(self, image):
        t = int(image[0, 0, 0])
        assert bool((image == t).all())
        self.seen.append(t)
        ids, uv = self.visible(t)
        return uv[ids].contiguous(), self.desc[ids].contiguous()


class Scorer:
    """Once the second lap begins: the first-lap keyframe nearest in truth pose."""

    def __init__(self, net, slam):
        self.net, self.slam, self.asked = net, slam, []

    def insert_and_query(self, n, image):
        ts = self.slam.tstamps_[:n + 1].tolist()
        t = ts[n]
        assert int(image[0, 0, 0]) == t  # the frame that waited under index n is keyframe n
        self.asked.append((n, t))
        first = [k for k in range(n) if ts[k] < LAP]
        if t < LAP or not first:
            return 0.0, 0
        c = self.net.gt_poses_t[:, :3]
        dist = [float((c[ts[k]] - c[t]).norm()) for k in first]
        return 1.0, first[int(np.argmin(dist))]


def _backend(net, dev):
    from dpvo_amd.long_term import LongTermLoopClosure

    class Recording(LongTermLoopClosure):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.estimated, self.closed, self.dropped = [], [], []

        def keyframe(self, k):
            self.dropped.append(k)
            super().keyframe(k)

        def estimate_3d_keypoints(self, i):
            out = super().estimate_3d_keypoints(i)
            self.estimated.append((i, int(self.slam.tstamps_[i]), out))
            return out

        def close_loop(self, i, j, n):
            first = len(self.estimated)
            ok = super().close_loop(i, j, n)
            self.closed.append((i, j, n, ok, self.estimated[first:]))
            return ok

    det = Detector(net, dev)
    return det, lambda cfg, slam: Recording(cfg, slam, det, Scorer(net, slam),
                                            generator=torch.Generator(device=dev).manual_seed(3))


TRACKER = dict(ba_iterations=1)  # keywords of the DPVO constructor


def _run(gpu, classic, **kw):
    from dpvo_amd import DPVO

    net = StandIn(gpu, FRAMES, motion=LAP)
    det, factory = _backend(net, gpu)
    cfg = _cfg(CLASSIC_LOOP_CLOSURE=classic, BUFFER_SIZE=128, **(kw or KEEP))
    slam = DPVO(cfg, net, ht=HT, wd=WD, device=gpu, **TRACKER,
                generator=torch.Generator(device=gpu).manual_seed(1), loop_closure=factory)
    net.slam = slam
    for t in range(FRAMES):
        slam(float(t), _image(gpu, t), _K(gpu))
    return slam, net, det


def _ratio_spread(det, t, kp):
    """Kept points against the landmarks in the camera of timestamp t: (scale,
    relative spread of the ratio = its standard deviation over its mean, number
    kept, smallest cosine, largest relative deviation from the median ratio)."""
    tr = kp.tracks
    ids, _ = det.visible(t)
    k = int(tr.count)
    sel = tr.sel[:k]
    got = tr.points[sel]
    truth = det.camera(t)[ids[sel]]
    ratio = got.norm(dim=1) / truth.norm(dim=1)
    scale = float(ratio.median())
    # direction too: the points are the landmarks, not just as far away
    cos = (got * truth).sum(1) / (got.norm(dim=1) * truth.norm(dim=1))
    return (scale, float(ratio.std() / ratio.mean()), k, float(cos.min()),
            float((ratio / scale - 1).abs().max()))


def test_loop_is_closed_and_the_trajectory_keeps_its_accuracy(gpu):
    """Two laps; the first candidate, keyframes (24, 1) at timestamps (31, 1), is
    closed.  Measured on the MI355X (the test prints every figure before it
    asserts): 96 of 118 keypoints kept in both frames, relative spread of the
    point ratio 9.1e-4 / 1.6e-3 (bound 1e-2), Sim(3) angle 1.0e-3 rad (bound
    6.4e-2), translation error 4.5e-3 (bound 0.13), scale error 2.5e-3, 96
    inliers; scale-aligned trajectory error 0.02655 with the closure, 0.02616
    without (allowance 1.5 x + 1e-3).  With _cfg's OPTIMIZATION_WINDOW of 4 the
    first frames stay 8e-2 off (spread) and the same closure makes the
    trajectory worse (0.165 against 0.041): the measurement is only as good
    as the map it is taken from."""
    slam, net, det = _run(gpu, True)
    lc = slam.long_term_lc
    assert slam.is_initialized and slam.counter == FRAMES
    print(f"n = {slam.n}, dropped keyframes {lc.dropped}, lc_count {lc.lc_count}")
    for i, j, n_at, ok, ests in lc.closed:
        print(f"  candidate ({i}, {j}) at n = {n_at}: closed {ok}; keypoints / kept "
              f"{[(e[2].keypoints.shape[0], int(e[2].tracks.count)) for e in ests]}")
    for i, t, kp in lc.estimated:
        assert kp.tracks.points.shape[0] == kp.keypoints.shape[0] == kp.descriptors.shape[0]
    poses, _ = slam.terminate()
    assert lc.lc_count >= 1
    i, j, n_at, ok, ests = next(c for c in lc.closed if c[3])
    assert i > j >= 1 and lc.loop_ii.tolist()[0] == i and lc.loop_jj.tolist()[0] == j

    # 3-D keypoints: the landmarks in camera i up to one common scale
    (ei, ti, kpi), (ej, tj, kpj) = ests
    assert (ei, ej) == (i, j) and ti >= LAP > tj
    si, spread_i, ki, cos_i, dev_i = _ratio_spread(det, ti, kpi)
    sj, spread_j, kj, cos_j, dev_j = _ratio_spread(det, tj, kpj)
    print(f"loop ({i}, {j}) at timestamps ({ti}, {tj}): kept {ki} / {kj} keypoints, scale "
          f"{si:.4f} / {sj:.4f}, relative spread {spread_i:.2e} / {spread_j:.2e} (largest "
          f"deviation {dev_i:.2e} / {dev_j:.2e}), min cosine {cos_i:.6f} / {cos_j:.6f}")

    # the Sim(3) measurement against the truth: X_j = X_i + (c_j - c_i), no rotation.  Points
    # within eps = 1e-2 of the scaled truth are off by at most delta = eps max|X|; a similarity
    # fitted to them is off by at most delta at the centroid and delta / r_rms in angle, hence
    # delta + angle |centroid| in translation at the origin.
    est = lc.last_estimate
    Xj = det.camera(tj)
    ids_j, _ = det.visible(tj)
    cloud = Xj[ids_j[kpj.tracks.sel[:kj]]]
    centroid = cloud.mean(0)
    r_rms = float((cloud - centroid).norm(dim=1).square().mean().sqrt())
    delta = 1e-2 * float(cloud.norm(dim=1).max())
    angle_tol = delta / r_rms
    t_tol = delta + angle_tol * float(centroid.norm())
    R = est.R.double().cpu().numpy()
    angle = float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))
    t_true = (net.gt_poses_t[tj, :3] - net.gt_poses_t[ti, :3]).cpu().numpy()
    t_err = float(np.linalg.norm(est.t.double().cpu().numpy() / sj - t_true))
    s_err = abs(float(est.s) / (sj / si) - 1)
    print(f"Sim(3): angle {angle:.2e} rad (bound {angle_tol:.2e}), translation error {t_err:.2e} "
          f"(bound {t_tol:.2e}, |t| {np.linalg.norm(t_true):.3f}), scale error {s_err:.2e}, "
          f"inliers {int(est.num_inliers)}")

    # the trajectory: no worse than the same run without the closure
    truth = net.truth_inverse(slam.counter)
    e_lc, s_lc = _scaled_error(poses, truth)
    slam0, net0, _ = _run(gpu, False)
    assert slam0.long_term_lc is None
    poses0, _ = slam0.terminate()
    e_0, s_0 = _scaled_error(poses0, net0.truth_inverse(slam0.counter))
    print(f"scale-aligned trajectory error: with the closure {e_lc:.5f} (scale {s_lc:.3f}), "
          f"without {e_0:.5f} (scale {s_0:.3f})")
    # every figure is printed above; the assertions follow
    assert ki >= 30 and kj >= 30
    assert spread_i < 1e-2 and spread_j < 1e-2
    assert cos_i > 1 - 1e-4 and cos_j > 1 - 1e-4
    assert angle <= angle_tol and t_err <= t_tol and s_err <= 2e-2
    assert int(est.num_inliers) >= 30
    assert np.isfinite(poses).all()
    assert e_lc <= 1.5 * e_0 + 1e-3


def test_cached_frames_follow_the_keyframe_drops(gpu):
    """Every frame the cache hands out by keyframe index carries that
    keyframe's timestamp, after drops moved the indices (the scorer asserts the
    same for the retrieval log on every insert)."""
    slam, net, det = _run(gpu, True, **DROP)
    lc = slam.long_term_lc
    print(f"n = {slam.n}, drops {len(lc.dropped)}, frames scored {len(lc.retrieval.scorer.asked)}")
    assert len(lc.dropped) > 0 and len(lc.retrieval.scorer.asked) > 10
    last = max(lc.imcache._saved)
    ts = slam.tstamps_[:last + 1].tolist()
    for k in range(1, last, 3):
        frames = lc.imcache.load_frames([k - 1, k, k + 1])
        assert frames[:, 0, 0, 0].tolist() == [t % 256 for t in ts[k - 1:k + 2]]
    table = lc.imcache.slot_of_frame[:slam.n, 0].tolist()
    assert table == [lc.imcache._slot[k] for k in range(slam.n)]


def test_without_a_backend_the_flag_still_raises_and_without_the_flag_nothing_is_called(gpu):
    from dpvo_amd import DPVO

    with pytest.raises(NotImplementedError, match="close_loop"):
        DPVO(_cfg(CLASSIC_LOOP_CLOSURE=True), StandIn(gpu, 4), ht=HT, wd=WD, device=gpu)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the backend was touched: {name}")

        def __call__(self, *a, **kw):
            raise AssertionError("the backend was called")

    net = StandIn(gpu, 12)
    slam = DPVO(_cfg(), net, ht=HT, wd=WD, device=gpu, loop_closure=Untouchable(),
                generator=torch.Generator(device=gpu).manual_seed(1))
    net.slam = slam
    for t in range(12):
        slam(float(t), _image(gpu, t), _K(gpu))
    poses, _ = slam.terminate()
    assert slam.long_term_lc is None and np.isfinite(poses).all()
