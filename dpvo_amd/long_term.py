"""The front half of the long-term ("classic") loop closure: from raw frames
to the matched 3-D points that `loop_closure.close_loop` starts from.

Restates dpvo/loop_closure/long_term.py `LongTermLoopClosure` and the
book-keeping of dpvo/loop_closure/retrieval (cuteboyqq/DPVO) without their
learned or external parts.  DISK, LightGlue and DBoW2 stay the caller's:

  detector(image uint8 [3, H, W]) -> (keypoints [K, 2] float32 image pixels,
                                      descriptors [K, D] float32 / float16)
  scorer.insert_and_query(n, image) -> (score, j) with j < n

and this module provides everything between them and `loop_closure`:

  `match_descriptors`    mutual nearest neighbours with a ratio test, the usual
                         stand-in for LightGlue on DISK descriptors
                         (`cuda_ba.match_descriptors`, match.hip: two launches);
  `triangulate_tracks`   `estimate_3d_keypoints` after the matcher: the tracks
                         over the frames i-1, i, i+1, the structure-only BA
                         that triangulates them, the residual and depth gates
                         and the un-projection (`cuda_ba.triangulate_tracks`,
                         triangulate.hip: one launch);
  `FrameCache`           the reference's ImageCache as device slots;
  `RetrievalLog`         RetrievalDBOW's frame queue, index shift, NMS and
                         consecutive-hit check around the caller's scorer;
  `LongTermLoopClosure`  the object `DPVO(cfg, net, loop_closure=...)` drives
                         when cfg.CLASSIC_LOOP_CLOSURE is set.

What differs from the reference: the pose-graph optimiser runs synchronously
(a few device launches; no worker pool, result queue or lc_in_progress), the
tracks are not shuffled (the reference's randperm only permutes LightGlue's
input), and the frames are cached raw on the device, not as JPEG files.
"""
from __future__ import annotations

from collections import deque
from typing import NamedTuple

import torch

from . import loop_closure
from ._native import load_extension, require_gpu
from .frontend import _scalar


class Matches(NamedTuple):
    """Result of `match_descriptors`, device tensors."""
    partner0: torch.Tensor  # [N0] int64: the matched row of desc1, or -1
    partner1: torch.Tensor  # [N1] int64: the matched row of desc0, or -1
    matches: torch.Tensor   # [min(N0, N1), 2] int64: pairs by ascending i, then -1
    dist2: torch.Tensor     # [min(N0, N1)] float32: squared distance of each pair, then -1
    count: torch.Tensor     # [] int32: the number of pairs


class Tracks(NamedTuple):
    """Result of `triangulate_tracks`, device tensors over the keypoints of frame i."""
    points: torch.Tensor  # [N1, 3] float32 camera-frame points (0 where no track)
    disp: torch.Tensor    # [N1] float32 final inverse depth (0 where no track)
    keep: torch.Tensor    # [N1] bool
    sel: torch.Tensor     # [N1] int64: the kept indices in ascending order, then -1
    count: torch.Tensor   # [] int32: the number kept


def match_descriptors(desc0, desc1, ratio=0.8, max_dist=float("inf"), n0=None, n1=None):
    """Mutual nearest neighbours of desc0 [N0, D] and desc1 [N1, D] with a
    ratio test -> `Matches`.

    float32, or float16 widened exactly; 1 <= N0, N1 <= 4096, D a multiple of 4
    in [4, 256].  n0 / n1 limit the valid rows (a Python int or an int32 device
    scalar, clamped to the rows present; None: all); rows at or beyond the
    limit are never read.  In fp32: sim = desc0 desc1^T (an fma chain over d
    ascending), d2 = max(|a|^2 + |b|^2 - 2 sim, 0).  Every row takes its best
    column (smaller d2, then the lower index) and the second-best d2 (+inf with
    one valid column), every column likewise; (i, j) is a match when each is
    the other's best, d2 <= float32(ratio^2) * second on both sides and d2 <=
    float32(max_dist^2).  Two launches, no host sync, no atomics: two runs are
    bit-equal, and the call can be captured into a graph."""
    ext = load_extension("cuda_ba")
    require_gpu(desc0)
    n0_host, n0_dev = _scalar(desc0.shape[0] if n0 is None else n0, "n0")
    n1_host, n1_dev = _scalar(desc1.shape[0] if n1 is None else n1, "n1")
    p0, p1, matches, dist2, count = ext.match_descriptors(
        desc0, desc1, float(ratio), float(max_dist), n0_host, n0_dev, n1_host, n1_dev)
    return Matches(p0, p1, matches, dist2, count[0])


def triangulate_tracks(poses, intrinsics, disps, kps0, kps1, kps2, m10, m12, max_depth=20.0,
                       max_residual=2.0, iterations=6, lmbda=1e-3):
    """The 3-D keypoints of frame i from its tracks over i-1, i, i+1
    (long_term.py:90-136 joined with the depth filter of :213-217) -> `Tracks`.

    poses [3, 7] and intrinsics [3, 4] of the three frames, the intrinsics at
    image resolution (the stored ones times RES); disps [M] (M <= 1024, any
    stride): the inverse depths patches_[i*M:(i+1)*M, 2, P//2, P//2]; kps0,
    kps1, kps2 [N, 2] float32 image pixels; m10 / m12 [N1] int64: `partner1`
    of match_descriptors(desc0, desc1) and of match_descriptors(desc2, desc1).
    A keypoint of frame i is a track when both partners are >= 0.  Its inverse
    depth starts at the lower median of disps (torch.median) and takes
    `iterations` steps dZ = u / (C + lmbda) of the structure-only BA over its
    two observations with weight 1, linearised, gated and clamped as
    fastba.BA does.  keep = both reprojection residuals < max_residual and
    points.z < max_depth (the reference filters by residual, then by depth;
    the surviving set is the same).  The reference's randperm of the tracks
    (long_term.py:90) only shuffles the order LightGlue sees them in and is not
    reproduced: the outputs are indexed by the keypoint of frame i.  One
    launch, no host sync."""
    ext = load_extension("cuda_ba")
    require_gpu(poses)
    points, disp, keep, sel, count = ext.triangulate_tracks(
        poses, intrinsics, disps, kps0, kps1, kps2, m10, m12, float(max_depth),
        float(max_residual), int(iterations), float(lmbda))
    return Tracks(points, disp, keep, sel, count[0])


class FrameCache:
    """The raw frames of the keyframes, uint8 [3, H, W], in device slots that
    never move (the reference's ImageCache writes JPEG files).

    `slot_of_frame` [N, 1] int32 maps a frame index to its slot (-1: none).
    It goes to `DevicePatchGraph.keyframe` as one more per-frame array with
    ring 0, so a keyframe drop moves four bytes per frame on the device;
    `keyframe(k)` does the same to the host's copy of the map and recycles the
    slot of the dropped frame.  `save_up_to(c)` marks the frames <= c as final,
    as the reference writes them to disk; only those can be loaded, and when
    all `capacity` slots are taken the oldest of them is evicted."""

    def __init__(self, capacity, num_frames, device=None):
        if capacity < 3:
            raise ValueError("FrameCache: capacity must hold a frame triplet")
        self.capacity = int(capacity)
        self.device = device
        self.slots = None
        self.slot_of_frame = None
        self._num_frames = int(num_frames)
        self._free = list(range(self.capacity - 1, -1, -1))
        self._slot = {}      # frame -> slot, the host's copy
        self._saved = set()  # frames that are final

    def _allocate(self, image):
        dev = image.device if self.device is None else torch.device(self.device)
        self.device = dev
        self.slots = torch.zeros((self.capacity,) + tuple(image.shape), dtype=torch.uint8,
                                 device=dev)
        self.slot_of_frame = torch.full((self._num_frames, 1), -1, dtype=torch.int32, device=dev)

    def table(self, image_shape, device):
        """The slot table, allocated before the first frame if need be."""
        if self.slots is None:
            self._allocate(torch.empty(image_shape, dtype=torch.uint8, device=device))
        return self.slot_of_frame

    def __contains__(self, n):
        return n in self._slot

    def __call__(self, image, n):
        if image.dtype != torch.uint8 or image.dim() != 3:
            raise TypeError("FrameCache: image must be uint8 [3, H, W]")
        if self.slots is None:
            self._allocate(image)
        slot = self._slot.get(n)
        if slot is None:
            if not self._free:
                if not self._saved:
                    raise RuntimeError(f"FrameCache: all {self.capacity} slots hold frames that "
                                       "are not final yet; increase the capacity")
                old = min(self._saved)
                self._saved.discard(old)
                self._free.append(self._slot.pop(old))
                self.slot_of_frame[old] = -1
            slot = self._free.pop()
            self._slot[n] = slot
            self.slot_of_frame[n] = slot
        self.slots[slot].copy_(image)

    def keyframe(self, k):
        """Frame k was dropped: frames above it move down by one.  The device
        table has been shifted by the patch graph's keyframe launch; this is
        the host's copy (and the free list)."""
        if k in self._slot:
            self._free.append(self._slot.pop(k))
        self._saved.discard(k)
        self._slot = {(n - 1 if n > k else n): s for n, s in self._slot.items()}
        self._saved = {(n - 1 if n > k else n) for n in self._saved}

    def shift_table(self, k):
        """The shift of `keyframe(k)` on the device table, for callers without
        a patch graph (the tracker's keyframe launch does it otherwise)."""
        t = self.slot_of_frame
        t[k:-1] = t[k + 1:].clone()

    def save_up_to(self, c):
        for n in self._slot:
            if n <= c:
                self._saved.add(n)

    def load_frames(self, idxs):
        """uint8 [len(idxs), 3, H, W] of final frames, gathered through the device table."""
        for n in idxs:
            if n not in self._saved:
                raise KeyError(f"FrameCache: frame {n} is not stored (evicted, dropped or not "
                               "final yet)")
        ix = torch.tensor(list(idxs), dtype=torch.long, device=self.slots.device)
        return self.slots[self.slot_of_frame[ix, 0].long()]


class RetrievalLog:
    """RetrievalDBOW's book-keeping (retrieval_dbow.py) around a caller's
    scorer, without its worker process: frames wait in a buffer until they can
    no longer be dropped, enter the scorer's database in `save_up_to`, and
    `detect_loop` reads the answers.

    scorer.insert_and_query(n, image) -> (score, j): the best earlier frame
    j < n for frame n, after n was added to the database."""

    def __init__(self, scorer, nms=50):
        self.scorer = scorer
        self.nms = nms
        self.image_buffer = {}
        self.stored_indices = set()
        self.prev_loop_closes = []
        self.found = []
        self._answers = deque()

    def __call__(self, image, n):
        self.image_buffer[n] = image

    def keyframe(self, k):
        """Frame k was dropped: forget it and move the waiting frames above it down."""
        tmp = dict(self.image_buffer)
        self.image_buffer.clear()
        for n, v in tmp.items():
            if n != k:
                self.image_buffer[(n - 1) if n > k else n] = v

    def save_up_to(self, c):
        for n in list(self.image_buffer):
            if n <= c:
                if n in self.stored_indices:
                    raise RuntimeError(f"RetrievalLog: frame {n} was stored before")
                image = self.image_buffer.pop(n)
                score, j = self.scorer.insert_and_query(n, image)
                self._answers.append((n, float(score), int(j)))
                self.stored_indices.add(n)

    def confirm_loop(self, i, j):
        if not i > j:
            raise ValueError("confirm_loop: i must be the later frame")
        self.prev_loop_closes.append((i, j))

    def _repetition_check(self, idx, num_repeat):
        """The pair in the middle of the last `num_repeat` hits when those came
        from consecutive frames (the reference unpacks exactly three); j = 0
        becomes 1, so that the triplet j-1, j, j+1 exists."""
        if len(self.found) < num_repeat:
            return None
        latest = self.found[-num_repeat:]
        b = latest[0][0]
        i, j = latest[num_repeat // 2]
        if (1 + idx - b) == num_repeat:
            return i, max(j, 1)
        return None

    def _detect_one(self, thresh, num_repeat):
        i, score, j = self._answers.popleft()
        if score < thresh:
            return None
        if not i > j:
            raise ValueError(f"RetrievalLog: the scorer answered j = {j} for frame {i}")
        near = [(i - a) ** 2 + (j - b) ** 2 for a, b in self.prev_loop_closes]
        if near and min(near) < self.nms ** 2:
            return None
        self.found.append((i, j))
        return self._repetition_check(i, num_repeat)

    def detect_loop(self, thresh, num_repeat=1):
        while self._answers:
            x = self._detect_one(thresh, num_repeat)
            if x is not None:
                return x
        return None


class Keypoints3D(NamedTuple):
    """`estimate_3d_keypoints`: the tracks of frame i and what they were made of."""
    tracks: Tracks
    keypoints: torch.Tensor    # [N1, 2] of frame i
    descriptors: torch.Tensor  # [N1, D] of frame i


class LongTermLoopClosure:
    """LongTermLoopClosure of the reference on the device ops of this package.

    slam: the `DPVO` it serves (poses_, patches_, intrinsics_, tstamps_, delta,
    M, N, P, RES are read, the first two written by a closure).  matcher: a
    function with the signature and result of `match_descriptors`."""

    MIN_NUM_INLIERS = 30

    def __init__(self, cfg, slam, detector, scorer, matcher=match_descriptors, cache_capacity=256,
                 nms=50, generator=None):
        self.cfg = cfg
        self.slam = slam
        self.detector = detector
        self.matcher = matcher
        self.retrieval = RetrievalLog(scorer, nms=nms)
        self.imcache = FrameCache(cache_capacity, slam.N, device=slam.dev)
        self.loop_ii = torch.zeros(0, dtype=torch.long, device=slam.dev)
        self.loop_jj = torch.zeros(0, dtype=torch.long, device=slam.dev)
        self.generator = generator
        self.lc_count = 0
        self.last_estimate = None

    def __call__(self, image, n):
        image = image.to(self.slam.dev)
        if image.dtype != torch.uint8:
            image = image.clamp(0, 255).to(torch.uint8)
        self.retrieval(image, n)
        self.imcache(image, n)

    def keyframe(self, k):
        self.retrieval.keyframe(k)
        self.imcache.keyframe(k)

    def frame_table(self):
        """The cache's slot table, for the per-frame arrays of the keyframe launch."""
        s = self.slam
        return self.imcache.table((3, s.ht, s.wd), s.dev)

    def estimate_3d_keypoints(self, i):
        """Detect, match and triangulate the keypoints of frame i over the
        triplet i-1, i, i+1 (long_term.py:70-138) -> Keypoints3D."""
        s = self.slam
        images = self.imcache.load_frames([i - 1, i, i + 1])
        (k0, d0), (k1, d1), (k2, d2) = (self.detector(im) for im in images)
        m10 = self.matcher(d0, d1).partner1
        m12 = self.matcher(d2, d1).partner1
        c = s.P // 2
        disps = s.patches_.view(s.N, s.M, 3, s.P, s.P)[i, :, 2, c, c]
        tracks = triangulate_tracks(s.poses_[i - 1:i + 2], s.intrinsics_[i - 1:i + 2] * s.RES,
                                    disps, k0, k1, k2, m10, m12)
        return Keypoints3D(tracks, k1, d1)

    def close_loop(self, i, j, n):
        """Try to close the loop (i, j) (long_term.py:205-267): True when the
        pose graph was optimised and the map corrected."""
        s = self.slam
        a = self.estimate_3d_keypoints(i)
        b = self.estimate_3d_keypoints(j)
        ta, tb = a.tracks, b.tracks
        # the kept descriptors first, their number as the matcher's row limit
        da = a.descriptors[ta.sel.clamp(min=0)]
        db = b.descriptors[tb.sel.clamp(min=0)]
        m = self.matcher(da, db, n0=ta.count.view(1), n1=tb.count.view(1))
        na, nb, nm = torch.stack([ta.count, tb.count, m.count]).tolist()  # the one host read
        if 3 * na < self.MIN_NUM_INLIERS:  # i_pts.numel(), as the reference compares it
            return False
        if 3 * nm < self.MIN_NUM_INLIERS:
            return False
        pairs = m.matches[:nm]
        i_pts = ta.points[ta.sel[pairs[:, 0]]]
        j_pts = tb.points[tb.sel[pairs[:, 1]]]
        out = loop_closure.close_loop(s.poses_, n, self.loop_ii, self.loop_jj, i, j, i_pts, j_pts,
                                      min_inliers=self.MIN_NUM_INLIERS, iterations=400,
                                      threshold=0.1, generator=self.generator)
        if out is None:
            return False
        final, self.loop_ii, self.loop_jj, self.last_estimate = out
        loop_closure.apply_result(final, s.poses_, s.patches_, n, s.M, delta=s.delta,
                                  tstamps=s.tstamps_)
        return True

    def attempt_loop_closure(self, n):
        cfg = self.cfg
        cands = self.retrieval.detect_loop(thresh=cfg.LOOP_RETR_THRESH,
                                           num_repeat=cfg.LOOP_CLOSE_WINDOW_SIZE)
        if cands is not None:
            i, j = cands
            closed = self.close_loop(i, j, n)
            self.lc_count += int(closed)
            if closed:  # no back-to-back detections of the same loop
                self.retrieval.confirm_loop(i, j)
            self.retrieval.found.clear()
        # frames that can no longer be dropped enter the database and the cache
        self.retrieval.save_up_to(n - cfg.REMOVAL_WINDOW - 2)
        self.imcache.save_up_to(n - cfg.REMOVAL_WINDOW - 1)

    def terminate(self, n):
        self.retrieval.save_up_to(n - 1)
        self.imcache.save_up_to(n - 1)
        self.attempt_loop_closure(n)


__all__ = ["Matches", "Tracks", "match_descriptors", "triangulate_tracks", "FrameCache",
           "RetrievalLog", "Keypoints3D", "LongTermLoopClosure"]
