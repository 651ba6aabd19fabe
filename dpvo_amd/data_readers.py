"""Training data on the device (csrc/dataset.hip): from a TartanAir directory to
the tensors ``train_step`` takes, without cv2, torchvision or a pickle.

frame_distance_matrix  rgbd_utils.compute_distance_matrix_flow: the mean flow
                       magnitude between every pair of frames, one launch.
build_frame_graph      base.py:64-82 -> FrameGraph (CSR on the device, .cpu(),
                       .row(i), .save / .load so a scene is built once).
read_disp              the host part of it (subsample, fill, invert), numpy.
sample_sequence        the index walk of base.py:98-138, both branches, numpy.
AugmentParams,         augmentation.py: the random draws are made on the host
RGBDAugmentor          into a record, the device work is a function of it.
normalize_depth        base.py:171-173, the quantile by a radix select.
RGBDDataset, TartanAir base.py / tartan.py: discovery, graph cache, __getitem__.

Two deviations from the reference, stated once here (and in DESIGN.md):

* The reference's colour path round-trips through PIL and quantises to uint8
  between the operations.  Here colour stays in fp32 and is not quantised; the
  formulas are in include/dpvo_hot.h.
* rgbd_utils.compute_distance_matrix_flow calls ``pops.induced_flow``, which the
  reference does not have.  The flow is defined through the reference's own
  ``projective_ops.transform(.., valid=True)`` on P = 1 patches.
"""
from __future__ import annotations

import dataclasses
import glob
import os
import os.path as osp

import numpy as np
import torch

from ._native import load_extension, require_gpu

JITTER_OPS = ("brightness", "contrast", "saturation", "hue")


# ---- frame graph ---------------------------------------------------------------------
def read_disp(depth, f=16):
    """base.py:66-69 on a depth map already read: subsample [f//2::f, f//2::f],
    depths below 0.01 take the mean of the subsampled map, then 1 / depth."""
    depth = np.array(depth[f // 2::f, f // 2::f])
    depth[depth < 0.01] = np.mean(depth)
    return 1.0 / depth


def frame_distance_matrix(poses, disps, intrinsics):
    """poses [N, 7] (world-from-camera, as the dataset stores them), disps
    [N, h, w], intrinsics [N, 4], float32 on the device -> D float32 [N, N]: the
    mean over both directions of min(|flow|, 100) over the points with Z > 0.2,
    +inf where fewer than 0.7 of the points are valid.  fp64 inside, symmetric
    bit for bit, one launch, no host synchronisation.  N <= 8192, h w <= 65536."""
    ext = load_extension("cuda_ba")
    require_gpu(poses)
    return ext.frame_flow_distance(poses, disps, intrinsics)


class FrameGraph:
    """CSR of the co-visible frames: row i holds the frames ``col`` (ascending)
    with flow distance ``dist`` < max_flow.  rowptr int32 [N + 1], col int32
    [nnz], dist float32 [nnz]."""

    def __init__(self, rowptr, col, dist):
        self.rowptr, self.col, self.dist = rowptr, col, dist

    def __len__(self):
        return int(self.rowptr.shape[0]) - 1

    def cpu(self):
        return FrameGraph(self.rowptr.cpu(), self.col.cpu(), self.dist.cpu())

    def row(self, i):
        """(j, d) of frame i as numpy arrays: ``graph[i]`` of the reference."""
        a, b = int(self.rowptr[i]), int(self.rowptr[i + 1])
        return self.col[a:b].cpu().numpy(), self.dist[a:b].cpu().numpy()

    @staticmethod
    def from_dense(d, max_flow=256):
        """The ``np.where`` loop of base.py:77-80 on a host matrix d (already
        times f)."""
        d = np.asarray(d)
        keep = d < max_flow
        rowptr = np.zeros(d.shape[0] + 1, dtype=np.int32)
        rowptr[1:] = np.cumsum(keep.sum(axis=1))
        _, col = np.nonzero(keep)
        return FrameGraph(torch.from_numpy(rowptr), torch.from_numpy(col.astype(np.int32)),
                          torch.from_numpy(d[keep].astype(np.float32)))

    def save(self, path):
        g = self.cpu()
        with open(path, "wb") as fh:
            np.savez(fh, rowptr=g.rowptr.numpy(), col=g.col.numpy(), dist=g.dist.numpy())

    @staticmethod
    def load(path):
        with np.load(path) as z:
            return FrameGraph(torch.from_numpy(z["rowptr"]), torch.from_numpy(z["col"]),
                              torch.from_numpy(z["dist"]))


def build_frame_graph(poses, disps, intrinsics, f=16, max_flow=256):
    """base.py:64-82 on the device: ``intrinsics`` already divided by f, ``disps``
    already ``read_disp``-subsampled.  d = f D in float32 (numpy's product), the
    entries d < max_flow as a FrameGraph on the device: a count, a scan and a
    fill launch, one host read of nnz to size the outputs."""
    ext = load_extension("cuda_ba")
    D = frame_distance_matrix(poses, disps, intrinsics)
    return FrameGraph(*ext.frame_graph(D, float(f), float(max_flow)))


# ---- sequence sampler ------------------------------------------------------------------
def sample_sequence(graph, ix, n_frames, fmin=10.0, fmax=75.0, sample=True, rng=None):
    """The index walk of base.py:98-138 from frame ix on a host FrameGraph ->
    the list of n_frames indices.  ``sample``: a random co-visible frame ahead
    (flow in (fmin, fmax)), else ix + 1, else any co-visible frame;
    otherwise the farthest frame within a drawn flow budget in the direction of
    travel, turning round at either end."""
    rng = np.random.default_rng() if rng is None else rng
    n = len(graph)
    d = rng.uniform(fmin, fmax)
    s = 1
    ix = int(ix)
    inds = [ix]
    while len(inds) < n_frames:
        j, g = graph.row(ix)
        if sample:
            frames = j[(g > fmin) & (g < fmax)]
            if np.count_nonzero(frames[frames > ix]):
                ix = int(rng.choice(frames[frames > ix]))
            elif ix + 1 < n:
                ix = ix + 1
            elif np.count_nonzero(frames):
                ix = int(rng.choice(frames))
        else:
            g = g.copy()
            g[g > d] = -1
            if s > 0:
                g[j <= ix] = -1
            else:
                g[j >= ix] = -1
            if len(g) > 0 and np.max(g) > 0:
                ix = int(j[np.argmax(g)])
            else:
                if ix + s >= n or ix + s < 0:
                    s *= -1
                ix = ix + s
        inds.append(ix)
    return inds


# ---- augmentation ----------------------------------------------------------------------
@dataclasses.dataclass
class AugmentParams:
    """The random draws of augmentation.py.  ``order``: the sequence of the four
    jitter operations as indices into JITTER_OPS (a permutation)."""
    do_color: bool = False
    order: tuple = (0, 1, 2, 3)
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0
    hue: float = 0.0
    gray: bool = False
    invert: bool = False
    scale: float = 1.0

    @staticmethod
    def draw(rng):
        """ColorJitter(0.4, 0.4, 0.4, 0.2 / 3.14) with p = 0.5, RandomGrayscale and
        RandomInvert with p = 0.1, scale 1 with p = 0.2 else 2 ** U(0, 0.5)."""
        p = AugmentParams()
        p.do_color = bool(rng.random() < 0.5)
        p.order = tuple(int(k) for k in rng.permutation(4))
        p.brightness, p.contrast, p.saturation = (float(v) for v in rng.uniform(0.6, 1.4, 3))
        p.hue = float(rng.uniform(-0.2 / 3.14, 0.2 / 3.14))
        p.gray = bool(rng.random() < 0.1)
        p.invert = bool(rng.random() < 0.1)
        p.scale = float(2.0 ** rng.uniform(0.0, 0.5)) if rng.random() < 0.8 else 1.0
        return p


class RGBDAugmentor:
    """augmentation.py's RGBDAugmentor on the device.

    aug(images [N, 3, H, W] float32 0..255, poses, disps [N, H, W], intrinsics
    [N, 4], rng=None, params=None) -> (images [N, 3, ch, cw], poses, disps
    [N, ch, cw], intrinsics): colour (jitter in ``params.order``, gray, invert),
    then resize by ``params.scale`` (bicubic image, nearest depth) and centre
    crop; only the crop window is computed.  ``params`` fixes every draw; else
    they come from ``rng`` (a numpy Generator).  swap_rb: plane 2 is red
    (cv2.imread's order, the reference's).  One to three launches, no host
    synchronisation; colour is fp32 and not quantised to uint8 between the
    operations as the reference's PIL path is."""

    def __init__(self, crop_size, swap_rb=True):
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.swap_rb = bool(swap_rb)

    def __call__(self, images, poses, disps, intrinsics, rng=None, params=None):
        ext = load_extension("cuda_ba")
        require_gpu(images)
        if params is None:
            params = AugmentParams.draw(np.random.default_rng() if rng is None else rng)
        images, disps, intrinsics = ext.rgbd_augment(
            images, disps, intrinsics, self.crop_size[0], self.crop_size[1], bool(params.do_color),
            [int(k) for k in params.order], float(params.brightness), float(params.contrast),
            float(params.saturation), float(params.hue), bool(params.gray), bool(params.invert),
            float(params.scale), self.swap_rb)
        return images, poses, disps, intrinsics


def normalize_depth(disps, poses, return_scale=False):
    """base.py:171-173: s = 0.7 torch.quantile(disps, 0.98) -> (disps / s, poses
    with the translation times s[, (s, lo, hi)]).  The two order statistics come
    from a radix select (no sort); s stays on the device."""
    ext = load_extension("cuda_ba")
    require_gpu(disps)
    disps, poses, s = ext.normalize_depth(disps, poses)
    return (disps, poses, s) if return_scale else (disps, poses)


# ---- readers ---------------------------------------------------------------------------
def read_split(split):
    """Scene names to hold out: a path to a file of names, or the names."""
    if split is None:
        return ()
    if isinstance(split, (str, os.PathLike)):
        with open(split) as fh:
            return tuple(fh.read().split())
    return tuple(split)


class RGBDDataset:
    """base.py's RGBDDataset: a video of n_frames co-visible frames per item.

    Subclasses give ``_build_scenes() -> {scene: {images, depths, poses,
    intrinsics}}`` and ``depth_read``.  The frame graph of a scene is built on
    the device once and cached as ``<cache>/<scene>.npz`` (cache=None: not kept).
    db[i] -> (images [1, n, 3, ch, cw] 0..255, poses [1, n, 7] world-from-camera
    -- ``train_step`` takes ``SE3(poses).inv()`` --, disps [1, n, ch, cw],
    intrinsics [1, n, 4]): float32 device tensors."""

    def __init__(self, datapath, n_frames=4, crop_size=(480, 640), fmin=10.0, fmax=75.0, aug=True,
                 sample=True, f=16, max_flow=256, cache=None, test_split=None, tail=65, bgr=True,
                 device="cuda", seed=None):
        self.root = str(datapath)
        self.n_frames, self.fmin, self.fmax = int(n_frames), float(fmin), float(fmax)
        self.sample, self.f, self.max_flow = bool(sample), int(f), max_flow
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.bgr = bool(bgr)
        self.aug = RGBDAugmentor(self.crop_size, swap_rb=self.bgr) if aug else None
        self.cache = None if cache is None else str(cache)
        self.test_split = read_split(test_split)
        self.tail = int(tail)
        self.device = torch.device(device)
        self.rng = np.random.default_rng(seed)
        self.scene_info = self._build_scenes()
        self._graphs = {}
        self._build_dataset_index()

    # -- what a dataset provides
    def _build_scenes(self):
        raise NotImplementedError

    @staticmethod
    def depth_read(depth_file):
        return np.load(depth_file)

    @staticmethod
    def image_read(image_file):
        """uint8 [H, W, 3] RGB as PIL decodes it."""
        from PIL import Image

        with Image.open(image_file) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)

    def is_test_scene(self, scene):
        return any(x in scene for x in self.test_split)

    # -- index
    def _build_dataset_index(self):
        self.dataset_index = []
        for scene, info in self.scene_info.items():
            if self.is_test_scene(scene):
                continue
            n = len(info["images"])
            self.dataset_index += [(scene, i) for i in range(n) if i < n - self.tail]

    def __len__(self):
        return len(self.dataset_index)

    def __imul__(self, x):
        self.dataset_index *= x
        return self

    # -- graph
    def _cache_file(self, scene):
        name = osp.relpath(scene, self.root).replace(os.sep, "_")
        return osp.join(self.cache, f"{name}_f{self.f}_m{self.max_flow}.npz")

    def scene_graph(self, scene):
        """The host FrameGraph of a scene: from memory, the cache, or the device."""
        if scene in self._graphs:
            return self._graphs[scene]
        path = self._cache_file(scene) if self.cache else None
        if path and osp.isfile(path):
            graph = FrameGraph.load(path)
        else:
            info = self.scene_info[scene]
            f = self.f
            disps = np.stack([read_disp(self.depth_read(fn), f) for fn in info["depths"]], 0)
            to = dict(device=self.device, dtype=torch.float32)
            graph = build_frame_graph(torch.as_tensor(np.asarray(info["poses"]), **to),
                                      torch.as_tensor(disps, **to),
                                      torch.as_tensor(np.asarray(info["intrinsics"]) / f, **to),
                                      f=f, max_flow=self.max_flow).cpu()
            if path:
                os.makedirs(self.cache, exist_ok=True)
                graph.save(path)
        self._graphs[scene] = graph
        return graph

    # -- item
    def _upload(self, images, depths, poses, intrinsics):
        """One pinned buffer, one copy: the float32 arrays first, the uint8 frames last
        (the host allocator keeps the buffer until the copy is over)."""
        parts = [np.ascontiguousarray(a, dtype=np.float32) for a in (depths, poses, intrinsics)]
        parts.append(np.ascontiguousarray(images, dtype=np.uint8))
        sizes = [a.nbytes for a in parts]
        pinned = torch.empty(sum(sizes), dtype=torch.uint8).pin_memory()
        host, o = pinned.numpy(), 0
        for a, nb in zip(parts, sizes):
            host[o:o + nb] = a.reshape(-1).view(np.uint8)
            o += nb
        dev = pinned.to(self.device, non_blocking=True)
        out, o = [], 0
        for a, nb in zip(parts, sizes):
            t = dev[o:o + nb]
            out.append((t.view(torch.float32) if a.dtype == np.float32 else t).view(a.shape))
            o += nb
        return out[3], out[0], out[1], out[2]

    def __getitem__(self, index, rng=None, params=None):
        rng = self.rng if rng is None else rng
        scene, ix = self.dataset_index[index % len(self.dataset_index)]
        info = self.scene_info[scene]
        inds = sample_sequence(self.scene_graph(scene), ix, self.n_frames, self.fmin, self.fmax,
                               self.sample, rng)
        images = np.stack([self.image_read(info["images"][i]) for i in inds])
        if self.bgr:
            images = images[..., ::-1]
        depths = np.stack([self.depth_read(info["depths"][i]) for i in inds])
        poses = np.stack([info["poses"][i] for i in inds])
        intrinsics = np.stack([info["intrinsics"][i] for i in inds])
        images, depths, poses, intrinsics = self._upload(images, depths, poses, intrinsics)
        images = images.permute(0, 3, 1, 2).float().contiguous()
        disps = 1.0 / depths
        if self.aug is not None:
            images, poses, disps, intrinsics = self.aug(images, poses, disps, intrinsics, rng=rng,
                                                        params=params)
        disps, poses = normalize_depth(disps, poses)
        return images[None], poses[None], disps[None], intrinsics[None]


class TartanAir(RGBDDataset):
    """tartan.py: scenes are the directories root/*/*/*/* with image_left/*.png,
    depth_left/*.npy and pose_left.txt; test_split names the held-out scenes."""

    DEPTH_SCALE = 5.0  # scale depths to balance rot & trans
    CALIB = (320.0, 320.0, 320.0, 240.0)

    def __init__(self, datapath, calib=None, **kwargs):
        self.calib = np.asarray(self.CALIB if calib is None else calib, dtype=np.float64)
        super().__init__(datapath, **kwargs)

    def _build_scenes(self):
        scene_info = {}
        for scene in sorted(glob.glob(osp.join(self.root, "*/*/*/*"))):
            images = sorted(glob.glob(osp.join(scene, "image_left/*.png")))
            depths = sorted(glob.glob(osp.join(scene, "depth_left/*.npy")))
            if len(images) != len(depths) or not images:
                continue
            poses = np.loadtxt(osp.join(scene, "pose_left.txt"), delimiter=" ").reshape(-1, 7)
            poses = poses[:, [1, 2, 0, 4, 5, 3, 6]]
            poses[:, :3] /= TartanAir.DEPTH_SCALE
            scene_info[scene] = {"images": images, "depths": depths, "poses": poses,
                                 "intrinsics": [self.calib] * len(images)}
        return scene_info

    @staticmethod
    def depth_read(depth_file):
        depth = np.load(depth_file) / TartanAir.DEPTH_SCALE
        depth[~np.isfinite(depth)] = 1.0  # the reference's intent (its == nan never fires)
        return depth


__all__ = ["read_disp", "frame_distance_matrix", "FrameGraph", "build_frame_graph",
           "sample_sequence", "AugmentParams", "RGBDAugmentor", "normalize_depth", "RGBDDataset",
           "TartanAir", "JITTER_OPS"]
