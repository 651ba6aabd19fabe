"""Frame preparation (undistort, halve, crop) in numpy on the CPU: the
comparison oracle of test_stream_ref.py and test_stream_gpu.py.

Written from the contract in include/dpvo_hot.h (OpenCV's documented camera
model, the map quantised to 1/32 pixel, an integer bilinear blend with a zero
border, then the 2 x 2 mean of INTER_AREA at 1/2 and the top-left crop of
dpvo/stream.py).  Whole-array numpy in float64 / int64: numpy does not contract
a * b + c, so every operation rounds once, in the order written.  It shares no
code with dpvo_amd/csrc/stream.hip.
"""
import numpy as np

LIM = float(2 ** 30)


def crop_size(h1, w1):
    return h1 - h1 % 16, w1 - w1 % 16


def output_size(h0, w0, scale):
    h1, w1 = (h0 // 2, w0 // 2) if scale == 0.5 else (h0, w0)
    return crop_size(h1, w1)


def distortion_map(calib, h0, w0):
    """(mx, my) float64 [h0, w0]: where undistorted pixel (u, v) reads the source."""
    c = np.zeros(9)
    c[:len(calib)] = np.asarray(calib, np.float64)
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = c
    u = np.arange(w0, dtype=np.float64)[None, :]
    v = np.arange(h0, dtype=np.float64)[:, None]
    x = (u - cx) / fx
    y = (v - cy) / fy
    r2 = x * x + y * y
    kr = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * kr + (2 * p1 * x * y + p2 * (r2 + 2 * x * x))
    yd = y * kr + (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
    return fx * xd + cx, fy * yd + cy


def quantise(m):
    """floor(m * 32 + 0.5) as int64, pinned to +-2^30 (NaN: -2^30); also the
    distance of m * 32 + 0.5 to the nearest integer (the floor's margin)."""
    s = m * 32 + 0.5
    q = np.floor(s)
    q = np.where(np.isnan(q), -LIM, q)
    q = np.clip(q, -LIM, LIM).astype(np.int64)
    margin = np.abs(s - np.round(s))
    return q, np.where(np.isnan(margin), 0.0, margin)


def taps(src, iy, ix):
    """src[iy, ix] with 0 outside; src [h0, w0, C] -> int64 [..., C], inside mask."""
    h0, w0 = src.shape[:2]
    inside = (iy >= 0) & (iy < h0) & (ix >= 0) & (ix < w0)
    val = src[np.clip(iy, 0, h0 - 1), np.clip(ix, 0, w0 - 1)].astype(np.int64)
    return val * inside[..., None], inside


def undistort(src, calib):
    """src uint8 [h0, w0, C] -> dict(image uint8 [h0, w0, C], margin [h0, w0]
    (the smaller floor margin of the two map axes), all_outside bool [h0, w0])."""
    h0, w0 = src.shape[:2]
    mx, my = distortion_map(calib, h0, w0)
    qx, gx = quantise(mx)
    qy, gy = quantise(my)
    ix, ax, iy, ay = qx >> 5, qx & 31, qy >> 5, qy & 31
    acc = np.zeros(src.shape, np.int64)
    none = np.ones((h0, w0), bool)
    for dy, dx, w in ((0, 0, (32 - ax) * (32 - ay)), (0, 1, ax * (32 - ay)),
                      (1, 0, (32 - ax) * ay), (1, 1, ax * ay)):
        val, inside = taps(src, iy + dy, ix + dx)
        acc += w[..., None] * val
        none &= ~inside
    return dict(image=((acc + 512) >> 10).astype(np.uint8), margin=np.minimum(gx, gy),
                all_outside=none)


def prepare_frame(raw, calib, scale=1.0, swap_rb=False):
    """raw uint8 [h0, w0] or [h0, w0, 3] -> dict(image uint8 [3, H, W],
    intrinsics float32 [4], margin [H, W]: the smallest floor margin among the
    undistorted pixels under each output pixel (inf without a remap),
    all_outside [h0, w0] or None)."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and (raw.ndim == 2 or (raw.ndim == 3 and raw.shape[2] == 3))
    assert scale in (1.0, 0.5) and len(calib) in (4, 8, 9)
    h0, w0 = raw.shape[:2]
    assert scale == 1.0 or (h0 % 2 == 0 and w0 % 2 == 0)
    src = raw[..., None] if raw.ndim == 2 else raw
    margin = np.full((h0, w0), np.inf)
    all_outside = None
    if len(calib) > 4:
        r = undistort(src, calib)
        src, margin, all_outside = r["image"], r["margin"], r["all_outside"]
    if scale == 0.5:
        s = src.astype(np.int64)
        src = ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        margin = np.minimum(np.minimum(margin[0::2, 0::2], margin[0::2, 1::2]),
                            np.minimum(margin[1::2, 0::2], margin[1::2, 1::2]))
    H, W = crop_size(*src.shape[:2])
    assert H > 0 and W > 0
    src, margin = src[:H, :W], margin[:H, :W]
    if src.shape[2] == 1:
        src = np.repeat(src, 3, axis=2)
    elif swap_rb:
        src = src[..., ::-1]
    intrinsics = (np.asarray(calib[:4], np.float64) * scale).astype(np.float32)
    return dict(image=np.ascontiguousarray(src.transpose(2, 0, 1)), intrinsics=intrinsics,
                margin=margin, all_outside=all_outside)
