"""The DPVO tracker (dpvo/dpvo.py `DPVO`) on the MI355X ops.

    slam = DPVO(default_config(), network)
    for t, image, K in frames:
        slam(t, image, K)
    poses, tstamps = slam.terminate()

Every stage of a frame is a HIP kernel of this tree: the encoders, the frame's
gathers (tracker.frame_sample), the frame front-end (frontend.init_frame), the
pyramid insert, the device patch graph, reprojection + edge order + BA plan,
A-CORR, the update operator, the target write (tracker.update_targets), window
and global BA, the map read-out (tracker.map_points), the keyframe drop and the
trajectory read-out.  The class is eager: the host reads the edge count and the
frame count once per frame, as the reference does, and before initialisation
the motion probe's decision.

`network` is a `VONet`, a DPVO checkpoint (path or state dict) loaded into one,
or any object with `.patchify`, `.update`, `.DIM`, `.RES` and `.P`: with a
`VONet` the tracker runs the two encoders and frame_sample itself, with any
other object it calls `network.patchify(...)` as the reference does.

With cfg.CLASSIC_LOOP_CLOSURE the tracker drives a `long_term.LongTermLoopClosure`
given as `loop_closure=` (the object, or a callable (cfg, slam) -> one) at the
reference's four sites: the raw image of every frame, the index of a dropped
keyframe, an attempt after every tracked frame, and terminate.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import altcorr, fastba, frontend, global_ba, tracker
from .patchgraph import DevicePatchGraph
from .synthetic import channels_last

_BUFFER_MSG = 'The buffer size is too small. You can increase it using "--opts BUFFER_SIZE={}"'


def default_config():
    """The keys and defaults of the reference's dpvo/config.py as a plain
    namespace (attribute access, like the yacs node it stands for)."""
    return SimpleNamespace(
        BUFFER_SIZE=4096, CENTROID_SEL_STRAT="RANDOM", PATCHES_PER_FRAME=80, REMOVAL_WINDOW=20,
        OPTIMIZATION_WINDOW=12, PATCH_LIFETIME=12, KEYFRAME_INDEX=4, KEYFRAME_THRESH=12.5,
        MOTION_MODEL="DAMPED_LINEAR", MOTION_DAMPING=0.5, MIXED_PRECISION=True,
        LOOP_CLOSURE=False, BACKEND_THRESH=64.0, MAX_EDGE_AGE=1000, GLOBAL_OPT_FREQ=15,
        CLASSIC_LOOP_CLOSURE=False, LOOP_CLOSE_WINDOW_SIZE=3, LOOP_RETR_THRESH=0.04,
        MAX_EDGES=10000)


class DPVO:
    LEVELS = (1, 4)

    def __init__(self, cfg, network, ht=480, wd=640, device="cuda", ba_iterations=1,
                 generator=None, loop_closure=None):
        if cfg.CLASSIC_LOOP_CLOSURE and loop_closure is None:
            raise NotImplementedError(
                "CLASSIC_LOOP_CLOSURE: the retrieval backend is not part of the tracker; drive "
                "loop_closure.close_loop / loop_closure.apply_result from the caller")
        self.cfg = cfg
        self.dev = dev = torch.device(device)
        self.dtype = torch.half if cfg.MIXED_PRECISION else torch.float
        self._load_network(network)
        net = self.network
        self.DIM, self.RES, self.P = int(net.DIM), int(net.RES), int(net.P)
        self.is_initialized = False
        self.M = M = int(cfg.PATCHES_PER_FRAME)
        self.N = N = int(cfg.BUFFER_SIZE)
        self.ht, self.wd = int(ht), int(wd)
        self.ba_iterations = int(ba_iterations)
        self.generator = generator
        h, w = self.ht // self.RES, self.wd // self.RES
        P, DIM = self.P, self.DIM

        # state attributes
        self.tlist = []
        self.counter = 0
        self.n = 0
        self.m = 0
        self.ran_global_ba = set()
        self.pmem = self.mem = 36
        self.last_global_ba = torch.tensor([-1000], dtype=torch.int32, device=dev)
        if cfg.LOOP_CLOSURE:
            self.pmem = int(cfg.MAX_EDGE_AGE)

        # per-frame buffers (patchgraph.py:11-36)
        self.poses_ = torch.zeros(N, 7, device=dev)
        self.poses_[:, 6] = 1.0
        self.patches_ = torch.zeros(N * M, 3, P, P, device=dev)
        self.intrinsics_ = torch.zeros(N, 4, device=dev)
        self.tstamps_ = torch.zeros(N, dtype=torch.long, device=dev)
        self.colors_ = torch.zeros(N, M, 3, dtype=torch.uint8, device=dev)
        self.points_ = torch.zeros(N * M, 3, device=dev)
        self.ix = torch.arange(N, device=dev).repeat_interleave(M)

        # feature rings
        self.imap_ = torch.zeros(self.pmem, M, DIM, device=dev, dtype=self.dtype)
        self.gmap_ = torch.zeros(self.pmem, M, 128, P, P, device=dev, dtype=self.dtype)
        self.pyramid = [channels_last(torch.zeros(1, self.mem, 128, h // s, w // s, device=dev,
                                                  dtype=self.dtype)) for s in self.LEVELS]
        self.fmap1_, self.fmap2_ = self.pyramid

        self.pg = DevicePatchGraph(max_edges=int(cfg.MAX_EDGES), DIM=DIM, device=dev, net=True)
        self.lmbda = torch.tensor([1e-4], device=dev)

        # frame times by counter, and the pg.delta log (both grow with the run)
        self._cap = max(N, 64)
        self.times = torch.zeros(self._cap, dtype=torch.float64, device=dev)
        self.delta = (torch.zeros(self._cap, 7, device=dev),
                      torch.zeros(self._cap, 2, dtype=torch.long, device=dev),
                      torch.zeros(1, dtype=torch.int32, device=dev))
        # device scalars: {n, m} of keyframe(), the frame row of the inserts
        self._st = torch.zeros(2, dtype=torch.int32, device=dev)
        self._row = torch.zeros(1, dtype=torch.int32, device=dev)
        self.kf = torch.zeros(2, dtype=torch.int32, device=dev)
        self.kf_mag = torch.zeros(2, dtype=torch.float32, device=dev)
        self._new_patches = torch.zeros(M, 3, P, P, device=dev)
        self._loop_out = None
        self._arM = torch.arange(M, device=dev)
        # what the last frame did (read by tests and callers that log)
        self.last_coords = None
        self.last_depth = None
        self.last_probe = None
        self.last_root = None
        self.updates = 0
        self.global_ba_runs = 0
        # the long-term loop closure (dpvo.py:179-185): a long_term.LongTermLoopClosure, or a
        # callable (cfg, slam) -> one; never touched unless CLASSIC_LOOP_CLOSURE is set
        self.long_term_lc = None
        if cfg.CLASSIC_LOOP_CLOSURE:
            self.long_term_lc = (loop_closure if hasattr(loop_closure, "attempt_loop_closure")
                                 else loop_closure(cfg, self))

    # -- network ---------------------------------------------------------------
    def _load_network(self, network):
        from .net import VONet

        if isinstance(network, (str, bytes, dict)) or hasattr(network, "__fspath__"):
            network = VONet(dtype=self.dtype).load_checkpoint(network)
        for a in ("patchify", "update", "DIM", "RES", "P"):
            if not hasattr(network, a):
                raise TypeError(f"DPVO: network has no attribute {a!r}")
        if isinstance(network, torch.nn.Module):
            network = network.to(self.dev).eval()
        self.network = network
        self._native = isinstance(network, VONet)

    # -- the reference's views ---------------------------------------------------
    @property
    def poses(self):
        return self.poses_.view(1, self.N, 7)

    @property
    def patches(self):
        return self.patches_.view(1, self.N * self.M, 3, self.P, self.P)

    @property
    def intrinsics(self):
        return self.intrinsics_.view(1, self.N, 4)

    @property
    def points(self):
        return self.points_[:self.m]

    @property
    def colors(self):
        return self.colors_[:self.n]

    @property
    def imap(self):
        return self.imap_.view(1, self.pmem * self.M, self.DIM)

    @property
    def gmap(self):
        return self.gmap_.view(1, self.pmem * self.M, 128, self.P, self.P)

    # -- helpers ---------------------------------------------------------------
    def _grow(self):
        """Room for one more frame in `times` and one more record in the delta log."""
        if self.counter + 2 < self._cap:
            return
        cap = 2 * self._cap

        def grown(t):
            new = torch.zeros((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            new[:t.shape[0]] = t
            return new

        self.times = grown(self.times)
        self.delta = (grown(self.delta[0]), grown(self.delta[1]), self.delta[2])
        self._cap = cap

    def _rand(self, fn, *args, **kw):
        g = self.generator
        if g is None:
            return fn(*args, device=self.dev, **kw)
        return fn(*args, device=g.device, generator=g, **kw).to(self.dev)

    def _centres(self, image, h, w):
        """Patch centres [M, 2] (x, y), drawn as Patchifier.forward draws them
        (net.py:364-386), from the tracker's generator."""
        M = self.M
        strat = self.cfg.CENTROID_SEL_STRAT
        if strat == "RANDOM":
            x = self._rand(torch.randint, 1, w - 1, size=[1, M])
            y = self._rand(torch.randint, 1, h - 1, size=[1, M])
        elif strat == "GRADIENT_BIAS":
            from .net import Patchifier

            g = Patchifier._image_gradient(image[None, None])
            x = self._rand(torch.randint, 1, w - 1, size=[1, 3 * M])
            y = self._rand(torch.randint, 1, h - 1, size=[1, 3 * M])
            cand = torch.stack([x, y], dim=-1).float()
            g = altcorr.patchify(g[0, :, None].contiguous(), cand, 0).view(1, 3 * M)
            order = torch.argsort(g, dim=1)
            x = torch.gather(x, 1, order[:, -M:])
            y = torch.gather(y, 1, order[:, -M:])
        else:
            raise NotImplementedError(f"Patch centroid selection not implemented: {strat}")
        return torch.stack([x, y], dim=-1).float()[0].contiguous()

    def _sample(self, image):
        """Encoders + gathers of the new frame into ring row n: returns the
        level-1 feature map [128, h, w] and fills self._new_patches."""
        n, M, P = self.n, self.M, self.P
        if self._native:
            pf = self.network.patchify
            fmap = pf.fnet(image[None, None])[0, 0]
            imap = pf.inet(image[None, None])[0, 0]
            coords = self._centres(image, fmap.shape[-2], fmap.shape[-1])
            tracker.frame_sample(fmap, imap, image, coords, self.gmap_, self.imap_, self.colors_, n,
                                 patches_out=self._new_patches, res=self.RES)
            self.last_coords = coords
            return fmap
        fmap, gmap, imap, patches, _, clr = self.network.patchify(
            image[None, None], patches_per_image=M,
            centroid_sel_strat=self.cfg.CENTROID_SEL_STRAT, return_color=True)
        clr = (clr[0, :, [2, 1, 0]] + 0.5) * (255.0 / 2)
        self.colors_[n] = clr.to(torch.uint8)
        self.imap_[n % self.pmem] = imap.reshape(M, self.DIM).to(self.dtype)
        self.gmap_[n % self.pmem] = gmap.reshape(M, 128, P, P).to(self.dtype)
        self._new_patches.copy_(patches.reshape(M, 3, P, P))
        self.last_coords = self._new_patches[:, :2, P // 2, P // 2].clone()
        return fmap.reshape(128, fmap.shape[-2], fmap.shape[-1])

    def _corr(self, coords, kk, jj, order=None):
        return altcorr.corr_levels(self.gmap, self.pyramid, coords, kk % (self.M * self.pmem),
                                   jj % self.mem, 3, self.LEVELS, order=order)

    def _set_counts(self):
        self._st[0:1].fill_(self.n)
        self._st[1:2].fill_(self.m)

    def _edges(self):
        """__edges_forw + __edges_back (dpvo.py:838-903) for the current n."""
        n, M, r, dev = self.n, self.M, int(self.cfg.PATCH_LIFETIME), self.dev
        lo = max(n - r, 0)
        kf = torch.arange(M * lo, M * max(n - 1, 0), device=dev)
        jf = torch.full_like(kf, n - 1)
        cb = n - lo
        kb = ((n - 1) * M + self._arM).repeat_interleave(cb)
        jb = torch.arange(lo, n, device=dev).repeat(M)
        return torch.cat([kf, kb]), torch.cat([jf, jb])

    def _loop_edges(self, gated):
        cfg = self.cfg
        if self._loop_out is None:
            dev, cap = self.dev, 1000 * self.M
            self._loop_out = (torch.empty(cap, dtype=torch.long, device=dev),
                              torch.empty(cap, dtype=torch.long, device=dev),
                              torch.zeros(1, dtype=torch.int32, device=dev),
                              torch.empty(self.pg._ext.edges_loop_work_floats(), device=dev))
        kk, jj, cnt = self.pg.edges_loop(
            self.poses_, self.patches_, self.intrinsics_, self.ix, self._st, self.N, self.M,
            last_global_ba=self.last_global_ba if gated else None,
            removal_window=int(cfg.REMOVAL_WINDOW), max_edge_age=int(cfg.MAX_EDGE_AGE),
            global_opt_freq=int(cfg.GLOBAL_OPT_FREQ), keyframe_index=int(cfg.KEYFRAME_INDEX),
            backend_thresh=float(cfg.BACKEND_THRESH), out=self._loop_out)
        self.pg.append_factors_dev(self.ix, kk, jj, cnt)

    def _check_edges(self):
        if self.pg.errors & 1:
            raise RuntimeError(f"Too many edges: the active edges exceed MAX_EDGES="
                               f"{self.pg.max_edges}; increase MAX_EDGES")

    # -- dpvo.py:570-584 ---------------------------------------------------------
    def motion_probe(self):
        """Median flow of the last frame's patches into the new frame (a device scalar)."""
        n, m, M = self.n, self.m, self.M
        kk = torch.arange(m - M, m, device=self.dev)
        jj = torch.full_like(kk, n)
        ii = self.ix[kk]
        net = torch.zeros(1, M, self.DIM, device=self.dev)
        coords = fastba.reproject(self.poses_, self.patches_, self.intrinsics_, ii, jj, kk)
        corr = self._corr(coords, kk, jj)
        ctx = self.imap[:, kk % (M * self.pmem)]
        _, (delta, _, _) = self.network.update(net, ctx, corr, None, ii, jj, kk)
        return tracker.probe_median(delta)

    # -- dpvo.py:775-836 ---------------------------------------------------------
    def update(self):
        E = self.pg.num_edges
        if E == 0:
            return
        cfg, pg, n, M = self.cfg, self.pg, self.n, self.M
        ii, jj, kk = pg.ii[:E], pg.jj[:E], pg.kk[:E]
        t0 = max(n - int(cfg.OPTIMIZATION_WINDOW), 1) if self.is_initialized else 1
        poses, patches, intr = self.poses_, self.patches_, self.intrinsics_
        ws = None
        if fastba.cuda_ba.plan_supported(E, t0, n, self.P):
            coords, order, ws = fastba.reproject(poses, patches, intr, ii, jj, kk, mem=self.mem,
                                                 plan_window=(t0, n))
        else:
            coords, order = fastba.reproject(poses, patches, intr, ii, jj, kk, mem=self.mem)
        corr = self._corr(coords, kk, jj, order=order)
        ctx = self.imap[:, kk % (M * self.pmem)]
        net, (delta, weight, _) = self.network.update(pg.net[:, :E], ctx, corr, None, ii, jj, kk)
        pg.net[:, :E] = net
        tracker.update_targets(coords, delta, weight, pg.target, pg.weight, E)
        self.updates += 1

        if global_ba.needs_global_ba(pg, n, int(cfg.REMOVAL_WINDOW)) and n not in self.ran_global_ba:
            global_ba.run_global_ba(pg, poses, patches, intr, n, M, lmbda=self.lmbda,
                                    delta=self.delta[0])
            self.ran_global_ba.add(n)
            self.global_ba_runs += 1
        else:
            fastba.BA(poses, patches, intr, pg.target[:, :E], pg.weight[:, :E], self.lmbda, ii, jj,
                      kk, t0, n, M, self.ba_iterations, plan=ws)
        tracker.map_points(poses, patches, intr, self.ix, self.points_, self.m)

    # -- dpvo.py:601-693 ---------------------------------------------------------
    def keyframe(self):
        cfg, mem, pmem = self.cfg, self.mem, self.pmem
        frames = [self.colors_.view(self.N, -1)]
        rings = [0]
        for p in self.pyramid:  # channels-last storage [1, mem, H, W, C]
            frames.append(p.permute(0, 1, 3, 4, 2).reshape(mem, -1))
            rings.append(mem)
        frames += [self.imap_.view(pmem, -1), self.gmap_.view(pmem, -1)]
        rings += [pmem, pmem]
        if self.long_term_lc is not None:  # the frame cache's slot table moves with the frames
            frames.append(self.long_term_lc.frame_table())
            rings.append(0)
        n_before = self.n
        self._set_counts()
        self.pg.keyframe(self._st, self.poses_, self.patches_, self.intrinsics_, self.M,
                         frames=frames, rings=rings, tstamps=self.tstamps_,
                         keyframe_index=int(cfg.KEYFRAME_INDEX),
                         keyframe_thresh=float(cfg.KEYFRAME_THRESH), kf=self.kf, mag=self.kf_mag,
                         delta=self.delta)
        self.pg.remove_by_window_dev(self.ix, self._st[0:1], int(cfg.REMOVAL_WINDOW),
                                     loop_closure=bool(cfg.LOOP_CLOSURE),
                                     optimization_window=int(cfg.OPTIMIZATION_WINDOW))
        self.n, self.m = (int(v) for v in self._st.tolist())
        if self.long_term_lc is not None and self.n < n_before:  # dpvo.py:675-676
            self.long_term_lc.keyframe(n_before - int(cfg.KEYFRAME_INDEX))

    # -- dpvo.py:905-1030 --------------------------------------------------------
    @torch.no_grad()
    def __call__(self, tstamp, image, intrinsics):
        """Track one frame: image [3, H, W] (uint8 or float, 0..255),
        intrinsics [4] = (fx, fy, cx, cy) at image resolution."""
        if (self.n + 1) >= self.N:
            raise Exception(_BUFFER_MSG.format(self.N * 2))
        if image.dim() != 3 or image.shape[0] != 3 or tuple(image.shape[1:]) != (self.ht, self.wd):
            raise ValueError(f"DPVO: image must be [3, {self.ht}, {self.wd}], got "
                             f"{tuple(image.shape)}")
        if self.long_term_lc is not None:  # dpvo.py:908-909: the raw image
            self.long_term_lc(image, self.n)
        image = image.to(self.dev)
        image = (2 * (image / 255.0) - 0.5).float().contiguous()
        intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32).to(self.dev)
        n, M = self.n, self.M
        self._grow()

        fmap = self._sample(image)
        self.last_depth = None
        if not self.is_initialized:  # dpvo.py:960: one random depth per patch
            self.last_depth = self._rand(torch.rand, M)
            self._new_patches[:, 2] = self.last_depth.view(M, 1, 1)
        self.tlist.append(tstamp)
        self.times[self.counter:self.counter + 1].fill_(float(tstamp))
        frontend.init_frame(self.poses_, self.patches_, self.intrinsics_, self.tstamps_, self.times,
                            self._new_patches, intrinsics, n, self.counter, M,
                            motion_model=self.cfg.MOTION_MODEL,
                            damping=float(self.cfg.MOTION_DAMPING), res=float(self.RES),
                            median=self.is_initialized)
        self._row.fill_(n)
        altcorr.insert_frame_ring(fmap.to(self.dtype).contiguous(), self.pyramid, self._row,
                                  self.LEVELS)

        self.counter += 1
        self.last_probe = None
        if n > 0 and not self.is_initialized:
            self.last_probe = float(self.motion_probe().item())
            if self.last_probe < 2.0:
                frontend.append_delta(self.delta, self.counter - 1, self.counter - 2)
                return

        self.n += 1
        self.m += M
        self._set_counts()
        if self.cfg.LOOP_CLOSURE:
            self._loop_edges(gated=True)
        kk, jj = self._edges()
        self.pg.append_factors(self.ix, kk, jj)
        self._check_edges()

        if self.n == 8 and not self.is_initialized:
            self.is_initialized = True
            for _ in range(12):
                self.update()
        elif self.is_initialized:
            self.update()
            self.keyframe()
        if self.long_term_lc is not None:  # dpvo.py:1027-1028
            self.long_term_lc.attempt_loop_closure(self.n)

    # -- dpvo.py:385-417 ---------------------------------------------------------
    def _trajectory(self, inverse):
        traj, root, info = frontend.trajectory(self.poses_, self.tstamps_, self.n, self.delta,
                                               self.counter, inverse=inverse)
        self.last_root = root
        return traj

    def get_pose(self, t):
        """The pose of frame t (by counter) as an SE3, interpolated through the
        pg.delta log for frames that are no keyframes."""
        from .lietorch import SE3

        return SE3(self._trajectory(inverse=False)[int(t)])

    @torch.no_grad()
    def terminate(self):
        """Final updates and the trajectory -> (poses [counter, 7] float32,
        inverted as the reference returns them; tstamps float64)."""
        if self.long_term_lc is not None:  # dpvo.py:394-395
            self.long_term_lc.terminate(self.n)
        if self.cfg.LOOP_CLOSURE:
            self._set_counts()
            self._loop_edges(gated=False)
            self._check_edges()
        for _ in range(12):
            self.ran_global_ba.discard(self.n)
            self.update()
        poses = self._trajectory(inverse=True).cpu().numpy()
        return poses, np.array(self.tlist, dtype=np.float64)


__all__ = ["DPVO", "default_config"]
