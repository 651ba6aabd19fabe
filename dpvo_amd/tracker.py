"""The small kernels of the tracker's frame path (csrc/tracker.hip).

frame_sample    Patchifier.forward after the encoders (dpvo/net.py:388-399) and
                the ring / colour writes of DPVO.__call__ (dpvo.py:937-938,
                965-969), one launch.
probe_median    torch.quantile(delta.norm(dim=-1).float(), 0.5) of the motion
                probe (dpvo.py:584) as a device scalar.
update_targets  target = coords[..., P/2, P/2] + delta, weight = w written into
                the patch graph (dpvo.py:805-810).
map_points      the centre pixel of pops.point_cloud for the first m patches
                (dpvo.py:834-836).

Each is one launch on the current stream and never synchronises with the
host; counts are Python ints or int32 device scalars, as in frontend.init_frame.
"""
from __future__ import annotations

from ._native import load_extension, require_gpu
from .frontend import _scalar


def frame_sample(fmap, imap, image, coords, gmap_ring, imap_ring, colors, n, *, patches_out=None,
                 res=4):
    """Sample frame n's patches into the rings, in place -> patches [M, 3, P, P].

    fmap [128, h, w] / imap [DIM, h, w]: the encoders' float32 NCHW output;
    image [3, H, W]: the normalised float32 image; coords [M, 2]: integer-valued
    (x, y) centres, 1 <= x <= w - 2, 1 <= y <= h - 2.  gmap_ring [pmem, M, 128,
    P, P] and imap_ring [pmem, M, DIM] (float16 or float32, the float16 value
    rounded to nearest) get rows (n % pmem) M + m; colors [N, M, 3] (uint8)
    row n gets ((v + 0.5) * (255 / 2)) truncated for v = image at (res x +
    res / 2, res y + res / 2), stored B, G, R.  The returned patches are the
    (x, y, 1) grid of every patch, ready for frontend.init_frame.  Every
    output is an exact copy of its source; no other row is written."""
    ext = load_extension("cuda_ba")
    require_gpu(fmap)
    n_host, n_dev = _scalar(n, "n")
    if patches_out is None:
        P = gmap_ring.shape[-1]
        patches_out = fmap.new_empty(coords.shape[0], 3, P, P)
    ext.frame_sample(fmap, imap, image, coords, gmap_ring, imap_ring, patches_out, colors,
                     int(res), n_host, n_dev)
    return patches_out


def probe_median(delta):
    """Median of the row norms of delta [M, 2] (float32 or float16, widened
    first) as torch.quantile(..., 0.5) gives it: a float32 device scalar.
    M <= 1024; NaN if any norm is NaN."""
    ext = load_extension("cuda_ba")
    require_gpu(delta)
    return ext.probe_median(delta.reshape(-1, 2))


def update_targets(coords, delta, weight, pg_target, pg_weight, E):
    """pg_target[e] = coords[e, :, P/2, P/2] + float(delta[e]) and pg_weight[e] =
    float(weight[e]) for e < E, in place; rows >= E stay.  coords [1, E, 2, P, P]
    float32, delta / weight [1, E, 2] float32 or float16, pg_target / pg_weight
    the patch graph's [1, MAX_EDGES, 2] float32 buffers.  E: a Python int, or an
    int32 device scalar (clamped to the rows the arguments hold)."""
    ext = load_extension("cuda_ba")
    require_gpu(coords)
    e_host, e_dev = _scalar(E, "E")
    ext.update_targets(coords, delta, weight, pg_target, pg_weight, e_host, e_dev)


def map_points(poses, patches, intrinsics, ix, points, m):
    """points[k] = X.xyz / X.w, X = poses[ix[k]]^-1 * ((x - cx) / fx, (y - cy) /
    fy, 1, d) at the centre pixel of patch k, for k < m; rows >= m stay.
    poses [N, 7], patches [N * M, 3, P, P], intrinsics [N, 4], ix [N * M]
    (int64), points [N * M, 3] float32.  fp64 arithmetic; d = 0 divides."""
    ext = load_extension("cuda_ba")
    require_gpu(poses)
    m_host, m_dev = _scalar(m, "m")
    ext.map_points(poses, patches, intrinsics, ix, points, m_host, m_dev)


__all__ = ["frame_sample", "probe_median", "update_targets", "map_points"]
