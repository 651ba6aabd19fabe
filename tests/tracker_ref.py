"""CPU restatement (torch / numpy) of the tracker's small kernels
(csrc/tracker.hip) and of the tracker's bookkeeping (dpvo_amd/dpvo.py), written
from dpvo/dpvo.py and dpvo/net.py of the reference."""
import numpy as np
import torch


# ---- the four kernels ----------------------------------------------------------------

def color_chain(p):
    """uint8 pixel -> the uint8 the tracker stores: normalise (dpvo.py:917), then
    (clr + 0.5) * (255 / 2) -> uint8 (dpvo.py:937-938), every step a float32 torch op."""
    v = 2 * (p / 255.0) - 0.5
    return ((v + 0.5) * (255.0 / 2)).to(torch.uint8)


def normalise(image_u8):
    return 2 * (image_u8 / 255.0) - 0.5


def frame_sample(fmap, imap, image, coords, P=3, ring_dtype=torch.float32, res=4):
    """fmap [C,h,w], imap [DIM,h,w], image [3,H,W] (normalised), coords [M,2] ->
    gmap [M,C,P,P], imap [M,DIM] (ring dtype), patches [M,3,P,P], colors [M,3] uint8."""
    r = P // 2
    x, y = coords[:, 0].long(), coords[:, 1].long()
    off = torch.arange(P) - r
    yy = (y[:, None, None] + off[None, :, None]).expand(-1, P, P)
    xx = (x[:, None, None] + off[None, None, :]).expand(-1, P, P)
    g = fmap[:, yy, xx].permute(1, 0, 2, 3).contiguous().to(ring_dtype)
    im = imap[:, y, x].T.contiguous().to(ring_dtype)
    patches = torch.stack([xx.float(), yy.float(), torch.ones_like(xx, dtype=torch.float32)], 1)
    clr = image[:, res * y + res // 2, res * x + res // 2].T  # [M, 3]
    clr = (clr[:, [2, 1, 0]] + 0.5) * (255.0 / 2)
    return g, im, patches, clr.to(torch.uint8)


def probe_median(delta):
    return torch.quantile(delta.float().norm(dim=-1), 0.5)


def update_targets(coords, delta, w):
    P = coords.shape[-1]
    return coords[..., P // 2, P // 2] + delta.float(), w.float()


def quat_to_matrix(q):
    """unit quaternion (x, y, z, w) [.., 4] fp64 -> rotation matrices [.., 3, 3]"""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z)
    R[..., 0, 1] = 2 * (x * y - z * w)
    R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w)
    R[..., 1, 1] = 1 - 2 * (x * x + z * z)
    R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w)
    R[..., 2, 1] = 2 * (y * z + x * w)
    R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def map_points(poses, patches, intrinsics, ix, m):
    """numpy fp64: points [m, 3] of the centre pixel of the first m patches."""
    poses, patches, intrinsics = (np.asarray(a, np.float64) for a in (poses, patches, intrinsics))
    P = patches.shape[-1]
    c = P // 2
    f = np.asarray(ix)[:m]
    K = intrinsics[f]
    x, y, d = patches[:m, 0, c, c], patches[:m, 1, c, c], patches[:m, 2, c, c]
    X = np.stack([(x - K[:, 2]) / K[:, 0], (y - K[:, 3]) / K[:, 1], np.ones(m)], -1)
    R = quat_to_matrix(poses[f, 3:])
    t = poses[f, :3]
    # pose^-1 acts as R^T (X.xyz - t X.w); the point is that over X.w = d
    Y = np.einsum("kji,kj->ki", R, X - t * d[:, None])
    return Y / d[:, None]


# ---- bookkeeping -----------------------------------------------------------------------

def edges_forw(n, M, r):
    """(kk, jj) of __edges_forw (dpvo.py:838-872), n after the increment."""
    kk = list(range(M * max(n - r, 0), M * max(n - 1, 0)))
    return kk, [n - 1] * len(kk)


def edges_back(n, M, r):
    """(kk, jj) of __edges_back (dpvo.py:874-903): meshgrid 'ij', kk outer."""
    kk, jj = [], []
    for k in range(M * max(n - 1, 0), M * n):
        for j in range(max(n - r, 0), n):
            kk.append(k)
            jj.append(j)
    return kk, jj


def new_edges(n, M, r):
    kf, jf = edges_forw(n, M, r)
    kb, jb = edges_back(n, M, r)
    return kf + kb, jf + jb


class Bookkeeping:
    """n, m, counter, tstamps_ and the active edge list of the tracker as a
    function of the decisions it took: frame(probe_ok, drop) per call."""

    def __init__(self, M, lifetime, removal_window, keyframe_index):
        self.M, self.r, self.rw, self.ki = M, lifetime, removal_window, keyframe_index
        self.n = self.m = self.counter = 0
        self.initialized = False
        self.tstamps = {}
        self.edges = []  # (ii, jj, kk)
        self.updates = 0
        self.delta = []  # (t1, t0)

    def frame(self, probe_ok=True, drop=False):
        M = self.M
        self.tstamps[self.n] = self.counter
        self.counter += 1
        if self.n > 0 and not self.initialized and not probe_ok:
            self.delta.append((self.counter - 1, self.counter - 2))
            return
        self.n += 1
        self.m += M
        kk, jj = new_edges(self.n, M, self.r)
        self.edges += [(k // M, j, k) for k, j in zip(kk, jj)]
        if self.n == 8 and not self.initialized:
            self.initialized = True
            self.updates += 12
        elif self.initialized:
            self.updates += 1
            if drop:
                k = self.n - self.ki
                self.delta.append((self.tstamps[k], self.tstamps[k - 1]))
                kept = [(i, j, q) for (i, j, q) in self.edges if i != k and j != k]
                self.edges = [(i - (i > k), j - (j > k), q - M * (i > k)) for (i, j, q) in kept]
                for i in range(k, self.n - 1):
                    self.tstamps[i] = self.tstamps[i + 1]
                self.n -= 1
                self.m -= M
            self.edges = [e for e in self.edges if not e[0] < self.n - self.rw]

    def edge_arrays(self):
        e = np.asarray(self.edges, np.int64).reshape(-1, 3)
        return e[:, 0], e[:, 1], e[:, 2]
