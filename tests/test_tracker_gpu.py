"""GPU: the tracker class (dpvo_amd/dpvo.py) at 64 x 96 images (16 x 24 feature
maps), M = 8, PATCH_LIFETIME 3, REMOVAL_WINDOW 5, OPTIMIZATION_WINDOW 4,
BUFFER_SIZE 64, MAX_EDGES 2000.

The stand-in network packages UpdateHarness's synthetic scene: a truth by
timestamp, fixed patch centres, a synthetic fmap, and the oracle update
(delta = true reprojection - coords, weight 0.5)."""
import numpy as np
import pytest
import torch

import oracle
import tracker_ref as R

pytestmark = pytest.mark.gpu

HT, WD, M_, P_ = 64, 96, 8, 3
H4, W4 = HT // 4, WD // 4
# (fx, fy, cx, cy) at image resolution: a long lens, so that a few pixels of flow per frame
# (the motion probe asks for 2) come with a baseline that is small against the scene depth
K_IMAGE = [320.0, 320.0, 48.0, 32.0]


def _cfg(**kw):
    from dpvo_amd import default_config

    cfg = default_config()
    cfg.PATCHES_PER_FRAME, cfg.PATCH_LIFETIME, cfg.REMOVAL_WINDOW = M_, 3, 5
    cfg.OPTIMIZATION_WINDOW, cfg.BUFFER_SIZE, cfg.MAX_EDGES = 4, 64, 2000
    for k, v in kw.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


def _bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bit_equal(got, ref, what=""):
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), what
    np.testing.assert_array_equal(_bits(got), _bits(ref), what)


# ---- the stand-in network ------------------------------------------------------------
class StandIn:
    DIM, RES, P = 384, 4, 3

    def __init__(self, dev, frames, motion="line", still=False, seed=0):
        from dpvo_amd.synthetic import se3_exp

        g = torch.Generator().manual_seed(seed)
        T = frames + 2
        t = np.arange(T, dtype=np.float64)
        xi = np.zeros((T, 6))
        if motion == "line":  # sideways at an uneven speed: one probe falls below 2 px
            xi[:, 0] = 0.05 * t + 0.02 * np.sin(0.9 * t)
            xi[:, 2] = 0.008 * t
            xi[:, 4] = 0.002 * np.sin(0.3 * t)
        else:  # a circle in x / z that comes back to its start after `motion` frames
            a = 2 * np.pi * t / motion
            xi[:, 0] = 0.3 * np.sin(a)
            xi[:, 2] = 0.3 * (1 - np.cos(a))
        xi[0] = 0
        self.T = T
        self.gt_poses_t = torch.from_numpy(se3_exp(xi)).float().to(dev)
        self.cxy = torch.stack([torch.randint(1, W4 - 1, (T, M_), generator=g),
                                torch.randint(1, H4 - 1, (T, M_), generator=g)], -1).float().to(dev)
        self.gt_d = (torch.rand(T, M_, generator=g) * 0.8 + 0.4).to(dev)
        self.field = torch.randn(128, H4, W4, generator=g).to(dev)
        self.still = still
        self.t = 0
        self.slam = None

    def patchify(self, images, patches_per_image=80, centroid_sel_strat="RANDOM", return_color=False):
        from dpvo_amd import altcorr

        assert patches_per_image == M_ and return_color
        dev = self.field.device
        t, self.t = self.t, self.t + 1
        fmap = (0.25 * torch.sin(self.field + 0.37 * t))[None]  # [1, 128, h, w]
        coords = self.cxy[t][None]
        gmap = altcorr.patchify(fmap, coords, 1).view(1, M_, 128, P_, P_)
        imap = torch.zeros(1, M_, self.DIM, 1, 1, device=dev)
        off = torch.arange(P_, device=dev, dtype=torch.float32) - P_ // 2
        patches = torch.ones(1, M_, 3, P_, P_, device=dev)
        patches[0, :, 0] = coords[0, :, 0].view(-1, 1, 1) + off.view(1, 1, P_)
        patches[0, :, 1] = coords[0, :, 1].view(-1, 1, 1) + off.view(1, P_, 1)
        clr = torch.zeros(1, M_, 3, device=dev)
        index = torch.zeros(M_, dtype=torch.long, device=dev)
        return fmap[None], gmap, imap, patches, index, clr

    def update(self, net, ctx, corr, flow, ii, jj, kk):
        from dpvo_amd import fastba

        s = self.slam
        ts = s.tstamps_.clamp(0, self.T - 1)
        gt_poses = self.gt_poses_t[ts]
        gt_patches = s.patches_.clone()
        gt_patches[:, 2] = self.gt_d[ts].reshape(-1, 1, 1)  # [N, M] -> patch rows
        true = fastba.reproject(gt_poses, gt_patches, s.intrinsics_, ii, jj, kk)
        coords = fastba.reproject(s.poses_, s.patches_, s.intrinsics_, ii, jj, kk)
        delta = (true - coords)[..., P_ // 2, P_ // 2].contiguous()
        if self.still:
            delta = torch.zeros_like(delta)
        return net, (delta, torch.full_like(delta, 0.5), None)

    def truth_inverse(self, counter):
        from dpvo_amd.lietorch import SE3

        return SE3(self.gt_poses_t[:counter]).inv().data.double().cpu().numpy()


def _tracker(gpu, frames, cfg=None, **kw):
    from dpvo_amd import DPVO

    net = StandIn(gpu, frames, **kw)
    slam = DPVO(cfg or _cfg(), net, ht=HT, wd=WD, device=gpu,
                generator=torch.Generator(device=gpu).manual_seed(1))
    net.slam = slam
    return slam, net


def _image(gpu, t=0):
    return torch.full((3, HT, WD), t % 256, dtype=torch.uint8, device=gpu)


def _K(gpu):
    return torch.tensor(K_IMAGE, device=gpu)


def _scaled_error(traj, truth):
    """mean distance of the camera centres after the best global scale"""
    c, g = traj[:, :3].astype(np.float64), truth[:, :3]
    c0, g0 = c - c.mean(0), g - g.mean(0)
    s = float((c0 * g0).sum() / (c0 * c0).sum())
    return float(np.linalg.norm(s * c0 - g0, axis=1).mean()), s


def _run_standin(gpu, frames, check=True, **cfg):
    slam, net = _tracker(gpu, frames, cfg=_cfg(**cfg))
    book = R.Bookkeeping(M_, 3, 5, slam.cfg.KEYFRAME_INDEX)
    probes, drops = [], []
    for t in range(frames):
        was_init, updates0 = slam.is_initialized, slam.updates
        slam(float(t), _image(gpu, t), _K(gpu))
        ok = slam.last_probe is None or slam.last_probe >= 2.0
        drop = was_init and bool(slam.kf[0].item())
        book.frame(ok, drop)
        if slam.last_probe is not None:
            probes.append(round(slam.last_probe, 3))
        if was_init:
            drops.append(int(drop))
        if not check:
            continue
        assert (slam.n, slam.m, slam.counter) == (book.n, book.m, book.counter), t
        assert slam.is_initialized == book.initialized, t
        if slam.is_initialized and not was_init:  # exactly when n first reaches 8
            assert slam.n == 8 and slam.updates - updates0 == 12
        if not slam.is_initialized:
            assert slam.n < 8 and slam.updates == 0
        E = slam.pg.num_edges
        ii, jj, kk = book.edge_arrays()
        assert E == len(ii), t
        for got, ref, name in ((slam.pg.ii, ii, "ii"), (slam.pg.jj, jj, "jj"), (slam.pg.kk, kk, "kk")):
            np.testing.assert_array_equal(got[:E].cpu().numpy(), ref, f"{name} at frame {t}")
        np.testing.assert_array_equal(slam.tstamps_[:slam.n].cpu().numpy(),
                                      [book.tstamps[i] for i in range(book.n)])
    assert slam.updates == book.updates
    assert slam.pg.errors == 0
    return slam, net, book, probes, drops


def _oracle_ba(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, M, iterations,
               eff_impl=False, plan=None):
    """fastba.BA with the C oracle (ba_cuda.cu:433-582 restated) on the host."""
    P, K = oracle.ba(poses.cpu().numpy(), patches.cpu().numpy(), intrinsics.cpu().numpy(),
                     target.float().cpu().numpy(), weight.float().cpu().numpy(),
                     float(lmbda.reshape(-1)[0]), ii.cpu().numpy(), jj.cpu().numpy(),
                     kk.cpu().numpy(), int(t0), int(t1), int(iterations))
    poses.copy_(torch.from_numpy(P).to(poses.device))
    patches.copy_(torch.from_numpy(K).to(patches.device))
    return []


def test_standin_scene_bookkeeping_and_accuracy(gpu, monkeypatch):
    """30 frames: initialisation exactly at n == 8 with 12 updates; n, m, counter,
    the edge lists and tstamps_ equal the restated bookkeeping under the
    decisions the run took; terminate() is finite with every frame resolved;
    and the scale-aligned trajectory error lies within 25 % of the same run
    with oracle.ba doing every BA.

    The error itself is large in both runs (about 0.14 over a 1.5-long path,
    measured): with OPTIMIZATION_WINDOW 4 the twelve updates at n == 8 free
    poses 4..7 only (dpvo.py:818, is_initialized is already set) and with
    REMOVAL_WINDOW 5 the first of them is the reference's global BA from t0 = 0
    (dpvo.py:815), so the initialisation does not reach the truth at these
    sizes, whichever BA runs.  The test compares the two, as the issue asks."""
    import dpvo_amd.fastba as fastba

    frames = 30
    slam, net, book, probes, drops = _run_standin(gpu, frames)
    assert slam.is_initialized and slam.counter == frames
    poses, tstamps = slam.terminate()
    assert poses.shape == (slam.counter, 7) and poses.dtype == np.float32
    assert tstamps.dtype == np.float64 and tstamps.tolist() == [float(t) for t in range(frames)]
    assert np.isfinite(poses).all()
    assert (slam.last_root.cpu().numpy() >= 0).all()
    assert fastba.cuda_ba.check_status(slam.poses_) & ~1 == 0
    e_hip, s_hip = _scaled_error(poses, net.truth_inverse(slam.counter))
    print(f"probe medians {probes}; keyframe drops {drops}; n = {slam.n}")

    monkeypatch.setattr(fastba, "BA", _oracle_ba)
    slam_o, net_o, _, _, drops_o = _run_standin(gpu, frames, check=False)
    poses_o, _ = slam_o.terminate()
    e_ora, s_ora = _scaled_error(poses_o, net_o.truth_inverse(slam_o.counter))
    print(f"scale-aligned trajectory error: HIP {e_hip:.5f} (scale {s_hip:.3f}), "
          f"oracle BA {e_ora:.5f} (scale {s_ora:.3f}); oracle drops {drops_o}")
    assert abs(e_hip - e_ora) <= 0.25 * e_ora


def test_standin_scene_bookkeeping_without_drops(gpu):
    """KEYFRAME_THRESH far below the scene's flow: frames stay, n grows past the
    removal window and the window rule alone prunes the edge list."""
    slam, _, book, _, drops = _run_standin(gpu, 20, KEYFRAME_THRESH=0.05)
    print(f"keyframe drops {drops}; n = {slam.n}, edges {slam.pg.num_edges}")
    assert slam.n > 8 + 5 and 0 in drops
    assert slam.pg.num_edges_inac > 0


def test_no_motion_before_initialisation(gpu):
    frames = 5
    slam, _ = _tracker(gpu, frames, still=True)
    for t in range(frames):
        slam(float(t), _image(gpu, t), _K(gpu))
    assert slam.n == 1 and slam.m == M_ and slam.counter == 5 and not slam.is_initialized
    log, pairs, count = slam.delta
    assert int(count.item()) == 4
    assert pairs[:4].tolist() == [[t, t - 1] for t in range(1, 5)]  # records (t, t - 1), t = 2 .. 4 among them
    ident = torch.tensor([0.0, 0, 0, 0, 0, 0, 1])
    assert torch.equal(log[:4].cpu(), ident.expand(4, 7))
    poses, tstamps = slam.terminate()
    assert poses.shape == (5, 7) and len(tstamps) == 5
    from dpvo_amd.lietorch import SE3

    inv0 = SE3(slam.poses_[:1]).inv().data.cpu().numpy()
    np.testing.assert_array_equal(poses, np.repeat(inv0, 5, 0))
    assert (slam.last_root.cpu().numpy() == 0).all()


def test_limits(gpu):
    from dpvo_amd import DPVO

    # BUFFER_SIZE 4: the reference raises once n + 1 >= N
    slam, _ = _tracker(gpu, 12, cfg=_cfg(BUFFER_SIZE=4))
    raised = None
    for t in range(10):
        if slam.n + 1 >= 4:
            with pytest.raises(Exception, match="buffer size is too small"):
                slam(float(t), _image(gpu, t), _K(gpu))
            raised = t
            break
        slam(float(t), _image(gpu, t), _K(gpu))
    assert raised is not None and slam.n == 3
    # MAX_EDGES 100: 8 + 24 + 40 edges after three frames, 112 with the fourth
    slam, _ = _tracker(gpu, 12, cfg=_cfg(MAX_EDGES=100))
    with pytest.raises(RuntimeError, match="MAX_EDGES"):
        for t in range(10):
            slam(float(t), _image(gpu, t), _K(gpu))
    assert slam.n == 4 and slam.pg.num_edges == 72
    slam, _ = _tracker(gpu, 4)
    with pytest.raises(ValueError):
        slam(0.0, torch.zeros(3, HT, WD + 4, dtype=torch.uint8, device=gpu), _K(gpu))
    with pytest.raises(NotImplementedError, match="close_loop"):
        DPVO(_cfg(CLASSIC_LOOP_CLOSURE=True), StandIn(gpu, 4), ht=HT, wd=WD, device=gpu)


def test_determinism(gpu):
    out = []
    for _ in range(2):
        slam, _ = _tracker(gpu, 14)
        for t in range(14):
            slam(float(t), _image(gpu, t), _K(gpu))
        poses, tstamps = slam.terminate()
        out.append((poses, tstamps, slam.points.clone(), slam.n))
    assert out[0][3] == out[1][3]
    np.testing.assert_array_equal(_bits(torch.from_numpy(out[0][0])), _bits(torch.from_numpy(out[1][0])))
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert_bit_equal(out[0][2], out[1][2], "points")
    assert out[0][2].shape == (out[0][3] * M_, 3)


def test_get_pose_and_properties(gpu):
    """get_pose(t) is the uninverted row of the read-out terminate() inverts; the
    properties are the reference's views; the map points are the restated
    centre-pixel cloud of the first m patches."""
    from dpvo_amd.lietorch import SE3

    slam, _ = _tracker(gpu, 12)
    for t in range(12):
        slam(float(t), _image(gpu, t), _K(gpu))
    assert slam.poses.shape == (1, 64, 7) and slam.patches.shape == (1, 64 * M_, 3, P_, P_)
    assert slam.intrinsics.shape == (1, 64, 4)
    assert slam.points.shape == (slam.m, 3) and slam.colors.shape == (slam.n, M_, 3)
    assert slam.points.data_ptr() == slam.points_.data_ptr()
    slam.update()  # keyframe() moved the frame rows after the last read-out; update() ends with it
    ref = R.map_points(slam.poses_.cpu().numpy(), slam.patches_.cpu().numpy(),
                       slam.intrinsics_.cpu().numpy(), slam.ix.cpu().numpy(), slam.m)
    got = slam.points.cpu().numpy().astype(np.float64)
    ok = np.isfinite(ref).all(1)
    err = np.linalg.norm(got[ok] - ref[ok], axis=1)
    assert ok.any() and (err <= 1e-5 * np.maximum(1.0, np.linalg.norm(ref[ok], axis=1))).all()
    poses, _ = slam.terminate()
    for t in (0, 5, slam.counter - 1):
        inv = SE3(slam.get_pose(t).data.view(1, 7)).inv().data.cpu().numpy()[0]
        np.testing.assert_allclose(inv, poses[t], atol=2e-6, rtol=1e-5)
    # a keyframe's pose is its row of poses_
    k = slam.n - 1
    np.testing.assert_allclose(slam.get_pose(int(slam.tstamps_[k])).data.view(7).cpu().numpy(),
                               slam.poses_[k].cpu().numpy(), atol=1e-6)


@pytest.mark.parametrize("strat", ["RANDOM", "GRADIENT_BIAS"])
def test_centres_of_both_strategies_are_legal_and_seeded(gpu, strat):
    """VONet path, float image input: the centres of either strategy lie in
    [1, w - 2] x [1, h - 2], and two trackers on one seed draw the same ones."""
    from dpvo_amd import DPVO, VONet

    torch.manual_seed(5)
    net = VONet(dtype=torch.float16)
    image = torch.randint(0, 256, (3, HT, WD), generator=torch.Generator().manual_seed(6)).float()
    drawn = []
    for _ in range(2):
        slam = DPVO(_cfg(CENTROID_SEL_STRAT=strat), net, ht=HT, wd=WD, device=gpu,
                    generator=torch.Generator(device=gpu).manual_seed(8))
        slam(0.0, image.to(gpu), K_IMAGE)
        c = slam.last_coords.cpu()
        assert c.shape == (M_, 2) and (c == c.round()).all()
        assert (c[:, 0] >= 1).all() and (c[:, 0] <= W4 - 2).all()
        assert (c[:, 1] >= 1).all() and (c[:, 1] <= H4 - 2).all()
        assert slam.n == 1 and slam.gmap_.dtype == torch.float16
        centre = slam.patches_[:M_, :2, 1, 1].cpu()
        assert torch.equal(centre, c)
        drawn.append(c)
    assert torch.equal(drawn[0], drawn[1])
    with pytest.raises(NotImplementedError):
        DPVO(_cfg(CENTROID_SEL_STRAT="GRID"), net, ht=HT, wd=WD, device=gpu)(0.0, image.to(gpu), K_IMAGE)


def test_loop_closure_wiring(gpu):
    """A circle that returns to its start, GLOBAL_OPT_FREQ 4, MAX_EDGE_AGE 40
    (KEYFRAME_INDEX 2: edges_loop's target frames are [n - GLOBAL_OPT_FREQ,
    n - KEYFRAME_INDEX), empty at the default 4; KEYFRAME_THRESH 1 px keeps
    every frame, because reduce_edges only takes pairs 30 or more frames apart).
    No accuracy claim."""
    frames = 44
    cfg = _cfg(LOOP_CLOSURE=True, GLOBAL_OPT_FREQ=4, MAX_EDGE_AGE=40, KEYFRAME_INDEX=2,
               MAX_EDGES=8000, KEYFRAME_THRESH=1.0)
    slam, _ = _tracker(gpu, frames, cfg=cfg, motion=36)
    assert slam.pmem == 40 and slam.imap_.shape[0] == 40
    moved = 0
    for t in range(frames):
        before = int(slam.last_global_ba.item())
        slam(float(t), _image(gpu, t), _K(gpu))
        moved += int(slam.last_global_ba.item()) != before
    print(f"loop frames {moved}, global BA runs {slam.global_ba_runs}, n = {slam.n}, "
          f"edges {slam.pg.num_edges} + {slam.pg.num_edges_inac} inactive")
    assert moved >= 1
    assert slam.global_ba_runs >= 1
    assert slam.pg.errors == 0
    poses, _ = slam.terminate()
    assert poses.shape == (frames, 7) and np.isfinite(poses).all()


# ---- real modules: the tracker against the same frame rebuilt from the public ops ----
class Shadow:
    """DPVO.__call__ / update / keyframe (dpvo.py:775-836, 905-1030) restated in
    the reference's order from the public ops, the four new pieces from
    tracker_ref; centres and random depths are the tracker's draws."""

    def __init__(self, cfg, net, dev):
        from dpvo_amd.patchgraph import DevicePatchGraph
        from dpvo_amd.synthetic import channels_last

        self.cfg, self.net, self.dev = cfg, net, dev
        N, M = cfg.BUFFER_SIZE, M_
        self.N = N
        self.n = self.m = self.counter = 0
        self.init = False
        self.pmem = self.mem = 36
        self.poses_ = torch.zeros(N, 7, device=dev)
        self.poses_[:, 6] = 1
        self.patches_ = torch.zeros(N * M, 3, P_, P_, device=dev)
        self.intrinsics_ = torch.zeros(N, 4, device=dev)
        self.tstamps_ = torch.zeros(N, dtype=torch.long, device=dev)
        self.colors_ = torch.zeros(N, M, 3, dtype=torch.uint8, device=dev)
        self.ix = torch.arange(N, device=dev).repeat_interleave(M)
        self.imap_ = torch.zeros(self.pmem, M, 384, device=dev)
        self.gmap_ = torch.zeros(self.pmem, M, 128, P_, P_, device=dev)
        self.pyramid = [channels_last(torch.zeros(1, self.mem, 128, H4 // s, W4 // s, device=dev))
                        for s in (1, 4)]
        self.pg = DevicePatchGraph(max_edges=cfg.MAX_EDGES, DIM=384, device=dev, net=True)
        self.times = torch.zeros(N, dtype=torch.float64, device=dev)
        self.delta = (torch.zeros(N, 7, device=dev), torch.zeros(N, 2, dtype=torch.long, device=dev),
                      torch.zeros(1, dtype=torch.int32, device=dev))
        self.lmbda = torch.tensor([1e-4], device=dev)
        self.ran_global = set()

    def corr(self, coords, kk, jj):
        from dpvo_amd import altcorr

        return altcorr.corr_levels(self.gmap_.view(1, -1, 128, P_, P_), self.pyramid, coords,
                                   kk % (M_ * self.pmem), jj % self.mem, 3, (1, 4))

    def frame(self, tstamp, image_u8, K, coords, depth):
        from dpvo_amd import altcorr, fastba, frontend

        M, n, dev = M_, self.n, self.dev
        image = 2 * (image_u8[None, None] / 255.0) - 0.5
        fmap, gmap, imap, patches, _, clr = self.net.patchify(
            image, patches_per_image=M, return_color=True, coords=coords[None])
        # tracker_ref's colour chain on the gathered pixels
        px = image[0, 0].cpu()[:, (4 * coords[:, 1] + 2).long().cpu(), (4 * coords[:, 0] + 2).long().cpu()]
        assert_bit_equal(clr[0].cpu(), px.T.contiguous(), "patchify's colour gather")
        ref_clr = ((px.T[:, [2, 1, 0]] + 0.5) * (255.0 / 2)).to(torch.uint8)
        self.colors_[n] = ref_clr.to(dev)
        if not self.init:
            patches[:, :, 2] = depth.view(1, M, 1, 1)
        self.times[self.counter] = tstamp
        frontend.init_frame(self.poses_, self.patches_, self.intrinsics_, self.tstamps_, self.times,
                            patches, K, n, self.counter, M, motion_model=self.cfg.MOTION_MODEL,
                            damping=self.cfg.MOTION_DAMPING, res=4.0, median=self.init)
        self.imap_[n % self.pmem] = imap.reshape(M, 384)
        self.gmap_[n % self.pmem] = gmap.reshape(M, 128, P_, P_)
        altcorr.insert_frame_ring(fmap[0, 0].contiguous(), self.pyramid,
                                  torch.tensor([n], dtype=torch.int32, device=dev), (1, 4))
        self.counter += 1
        if n > 0 and not self.init:
            kk = torch.arange(self.m - M, self.m, device=dev)
            jj = torch.full_like(kk, n)
            ii = self.ix[kk]
            c = fastba.reproject(self.poses_, self.patches_, self.intrinsics_, ii, jj, kk)
            ctx = self.imap_.view(1, -1, 384)[:, kk % (M * self.pmem)]
            _, (delta, _, _) = self.net.update(torch.zeros(1, M, 384, device=dev), ctx,
                                               self.corr(c, kk, jj), None, ii, jj, kk)
            self.probe = float(R.probe_median(delta[0].cpu()))
            if self.probe < 2.0:
                frontend.append_delta(self.delta, self.counter - 1, self.counter - 2)
                return
        self.n += 1
        self.m += M
        kk, jj = R.new_edges(self.n, M, self.cfg.PATCH_LIFETIME)
        self.pg.append_factors(self.ix, torch.tensor(kk, device=dev), torch.tensor(jj, device=dev))
        if self.n == 8 and not self.init:
            self.init = True
            for _ in range(12):
                self.update()
        elif self.init:
            self.update()
            self.keyframe()

    def update(self):
        from dpvo_amd import fastba, global_ba

        pg, n, E = self.pg, self.n, self.pg.num_edges
        ii, jj, kk = pg.ii[:E], pg.jj[:E], pg.kk[:E]
        coords = fastba.reproject(self.poses_, self.patches_, self.intrinsics_, ii, jj, kk)
        ctx = self.imap_.view(1, -1, 384)[:, kk % (M_ * self.pmem)]
        net, (delta, weight, _) = self.net.update(pg.net[:, :E], ctx, self.corr(coords, kk, jj),
                                                  None, ii, jj, kk)
        pg.net[:, :E] = net
        target, weight = R.update_targets(coords.cpu(), delta.cpu(), weight.cpu())
        pg.target[:, :E] = target.to(self.dev)
        pg.weight[:, :E] = weight.to(self.dev)
        if global_ba.needs_global_ba(pg, n, self.cfg.REMOVAL_WINDOW) and n not in self.ran_global:
            global_ba.run_global_ba(pg, self.poses_, self.patches_, self.intrinsics_, n, M_,
                                    lmbda=self.lmbda, delta=self.delta[0])
            self.ran_global.add(n)
        else:
            t0 = max(n - self.cfg.OPTIMIZATION_WINDOW, 1) if self.init else 1
            fastba.BA(self.poses_, self.patches_, self.intrinsics_, pg.target[:, :E],
                      pg.weight[:, :E], self.lmbda, ii, jj, kk, t0, n, M_, 1)

    def keyframe(self):
        st = torch.tensor([self.n, self.m], dtype=torch.int32, device=self.dev)
        frames = [self.colors_.view(self.N, -1)]
        frames += [p.permute(0, 1, 3, 4, 2).reshape(self.mem, -1) for p in self.pyramid]
        frames += [self.imap_.view(self.pmem, -1), self.gmap_.view(self.pmem, -1)]
        self.pg.keyframe(st, self.poses_, self.patches_, self.intrinsics_, M_, frames=frames,
                         rings=[0, self.mem, self.mem, self.pmem, self.pmem], tstamps=self.tstamps_,
                         keyframe_index=self.cfg.KEYFRAME_INDEX,
                         keyframe_thresh=self.cfg.KEYFRAME_THRESH, delta=self.delta)
        self.n, self.m = (int(v) for v in st.tolist())
        self.pg.remove_by_window(self.ix, self.n, self.cfg.REMOVAL_WINDOW)


def test_real_modules_composition_parity(gpu):
    """VONet with seeded default-initialised fp32 weights over 11 seeded random
    images; the same frames rebuilt from the public ops give the same bits at
    frames 1, 8 and 11.  The bias of the last linear of update.d is set to
    (3.0, 1.0): with default weights the flow head gives well under a pixel, the
    motion probe (< 2 px) would reject every frame and the tracker would never
    initialise."""
    from dpvo_amd import DPVO, VONet, fastba

    torch.manual_seed(11)
    net = VONet(dtype=torch.float32)
    with torch.no_grad():
        net.update.d[1].bias.copy_(torch.tensor([3.0, 1.0]))
    cfg = _cfg(MIXED_PRECISION=False)
    slam = DPVO(cfg, net, ht=HT, wd=WD, device=gpu,
                generator=torch.Generator(device=gpu).manual_seed(2))
    shadow = Shadow(cfg, net, gpu)
    g = torch.Generator().manual_seed(4)
    K = _K(gpu)
    for f in range(1, 12):
        image = torch.randint(0, 256, (3, HT, WD), generator=g, dtype=torch.uint8).to(gpu)
        slam(0.1 * f, image, K)
        depth = slam.last_depth.clone() if slam.last_depth is not None else None
        shadow.frame(0.1 * f, image, K, slam.last_coords.clone(), depth)
        if f not in (1, 8, 11):
            continue
        assert (slam.n, slam.m, slam.counter) == (shadow.n, shadow.m, shadow.counter), f
        assert slam.is_initialized == shadow.init
        E = slam.pg.num_edges
        assert E == shadow.pg.num_edges
        for name in ("poses_", "patches_", "imap_", "gmap_", "tstamps_", "colors_"):
            assert_bit_equal(getattr(slam, name), getattr(shadow, name), f"{name} at frame {f}")
        for name in ("ii", "jj", "kk"):
            assert_bit_equal(getattr(slam.pg, name)[:E], getattr(shadow.pg, name)[:E], name)
        for name in ("net", "target", "weight"):
            assert_bit_equal(getattr(slam.pg, name)[:, :E], getattr(shadow.pg, name)[:, :E],
                             f"pg.{name} at frame {f}")
        status = fastba.cuda_ba.check_status(slam.poses_)
        print(f"frame {f}: n = {slam.n}, E = {E}, probe {slam.last_probe}, BA status {status}")
        assert status == 0, "the BA reported a failure at a compared frame"
        assert torch.isfinite(slam.poses_).all() and torch.isfinite(slam.patches_).all()
    assert slam.is_initialized and slam.n >= 8
