"""Pure numpy / torch restatements of csrc/dataset.hip for the tests, run on the
CPU: the frame flow distance in fp64, the colour map of the augmentor in a
chosen dtype, the spatial part through F.interpolate (torch is the definition
there), and the scenes and the synthetic TartanAir tree the tests share."""
import os

import numpy as np
import torch
import torch.nn.functional as F


# ---- frame flow distance (include/dpvo_hot.h, dpvo_frame_flow_distance) ----------------
def q_act(q, p):
    v = q[..., :3]
    uv = 2.0 * np.cross(v, p)
    return p + q[..., 3:4] * uv + np.cross(v, uv)


def pose_inv(t, q):
    qi = q * np.array([-1.0, -1.0, -1.0, 1.0])
    return -q_act(qi, t), qi


def pose_mul(ta, qa, tb, qb):
    x1, y1, z1, w1 = np.moveaxis(qa, -1, 0)
    x2, y2, z2, w2 = np.moveaxis(qb, -1, 0)
    q = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                  w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2,
                  w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)
    return ta + q_act(qa, tb), q


def flow_distance(poses, disps, intrinsics):
    """-> (D float32 [N, N], k int [N, N], near bool [N, N]): the matrix, the
    pooled count of valid points of every pair, and whether some point of the
    pair has |Z - 0.2| < 1e-6 (the only entries a test may exclude)."""
    P = np.asarray(poses, np.float32).astype(np.float64)
    d = np.asarray(disps, np.float32).astype(np.float64)
    K = np.asarray(intrinsics, np.float32).astype(np.float64)
    N, h, w = d.shape
    t, q = pose_inv(P[:, :3], P[:, 3:])          # G = inv(pose)
    ti, qi = pose_inv(t, q)                      # inv(G)
    # G_ab = G_b * inv(G_a) for every ordered pair [a, b]
    tab, qab = pose_mul(t[None, :], q[None, :], ti[:, None], qi[:, None])
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    fx, fy, cx, cy = (K[:, c] for c in range(4))
    X0 = np.stack([(x[None] - cx[:, None]) / fx[:, None], (y[None] - cy[:, None]) / fy[:, None],
                   np.ones((N, h * w))], -1)     # [a, p, 3]
    X1 = q_act(qab[:, :, None, :], X0[:, None]) + tab[:, :, None, :] * d.reshape(N, 1, -1, 1)
    Z = X1[..., 2]
    zc = np.maximum(Z, 0.1)
    u = fx[None, :, None] * (X1[..., 0] / zc) + cx[None, :, None]
    v = fy[None, :, None] * (X1[..., 1] / zc) + cy[None, :, None]
    mag = np.minimum(np.sqrt((u - x) ** 2 + (v - y) ** 2), 100.0)
    val = Z > 0.2
    s = (mag * val).sum(-1)
    k = val.sum(-1)
    s, k = s + s.T, k + k.T
    n = 2 * h * w
    with np.errstate(divide="ignore", invalid="ignore"):
        D = (s / k).astype(np.float32)
    D[(k.astype(np.float32) / np.float32(n)) < np.float32(0.7)] = np.inf
    near = (np.abs(Z - 0.2) < 1e-6).any(-1)
    return D, k, near | near.T


def _yaw(deg):
    a = np.deg2rad(deg) / 2
    return [0.0, np.sin(a), 0.0, np.cos(a)]


def share_counts(hw):
    """(k_above, k_below): the smallest pooled count that is not below the 0.7 share
    and the one under it, by the fp32 test (float)k / (float)n < 0.7f itself.  (At
    10 x 13 points 0.7 n = 182 is an integer; 182 / 260 rounds to 0.7f, which is
    not below 0.7f, on the device and in the restatement alike.)"""
    n = np.float32(2 * hw)
    ka = next(k for k in range(2 * hw + 1) if not (np.float32(k) / n < np.float32(0.7)))
    return ka, ka - 1


def make_scene(N, h, w, seed, pick=None):
    """poses [N, 7], disps [N, h, w], intrinsics [N, 4] (float32) and the roles of
    the special frames.  Frame `base` looks down +z; the others, by role:
      above / below  pure translations along z, far enough that exactly so many
                     of base's points fall behind Z = 0.2 that the pooled share
                     of valid points is just above / just below 0.7
      turn           a 180 degree turn on the spot: every point behind the camera
      clamp          a sideways translation of 100: every flow far above 100
      rot            a pure rotation (6 degrees of yaw)
      trans          a small sideways translation
    and N - len(pick) frames of a smooth random walk.  Intrinsics differ per frame."""
    rng = np.random.default_rng(seed)
    roles = ["base", "above", "below", "turn", "clamp", "rot", "trans"] if pick is None else pick
    assert roles[0] == "base" and N >= len(roles)
    hw = h * w
    disps = rng.uniform(0.3, 1.0, (N, h, w))
    ds = np.sort(disps[0].reshape(-1))[::-1]
    ka, kb = share_counts(hw)
    T = {}
    for name, k in (("above", ka), ("below", kb)):
        m = 2 * hw - k                              # base's points that must be invalid
        T[name] = 0.8 / (0.5 * (ds[m - 1] + ds[m]))  # 1 - T d <= 0.2 for the m largest d
    ident = [0.0, 0.0, 0.0, 1.0]
    special = {"base": [0, 0, 0] + ident, "above": [0, 0, T["above"]] + ident,
               "below": [0, 0, T["below"]] + ident, "turn": [0, 0, 0] + _yaw(180.0),
               "clamp": [100.0, 0, 0] + ident, "rot": [0, 0, 0] + _yaw(6.0),
               "trans": [0.05, 0, 0] + ident}
    poses = [special[r] for r in roles]
    p = np.zeros(3)
    for i in range(N - len(roles)):
        p = p + rng.normal(0, 0.04, 3)
        a = rng.normal(0, 0.03, 3)
        q = np.concatenate([a / 2, [1.0]])
        poses.append(list(p) + list(q / np.linalg.norm(q)))
    K = np.stack([np.array([w, w, w / 2, h / 2]) * (1 + 0.01 * (i % 7)) for i in range(N)])
    K[:, 2:] += rng.uniform(-0.3, 0.3, (N, 2))
    return (np.asarray(poses, np.float32), disps.astype(np.float32), K.astype(np.float32),
            {r: i for i, r in enumerate(roles)})


# ---- colour (include/dpvo_hot.h, dpvo_rgbd_augment) --------------------------------------
def _gray(r, g, b):
    return 0.299 * r + 0.587 * g + 0.114 * b


def _hue(r, g, b, delta):
    maxc = torch.maximum(r, torch.maximum(g, b))
    minc = torch.minimum(r, torch.minimum(g, b))
    cr = maxc - minc
    flat = cr == 0
    one = torch.ones_like(cr)
    crd = torch.where(flat, one, cr)
    s = torch.where(flat, torch.zeros_like(cr), cr / torch.where(flat, one, maxc))
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    h = torch.where(maxc == r, bc - gc, torch.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = torch.where(flat, torch.zeros_like(h), torch.fmod(h / 6.0 + 1.0, 1.0))
    h = h + delta
    h = h - torch.floor(h)
    v = maxc
    h6 = h * 6.0
    fl = torch.floor(h6)
    f = h6 - fl
    i = fl.to(torch.int64) % 6
    p, q, t = v * (1.0 - s), v * (1.0 - f * s), v * (1.0 - (1.0 - f) * s)
    pick = lambda *c: torch.stack(c, 0).gather(0, i[None])[0]  # noqa: E731
    return (pick(v, q, p, p, t, v).clamp(0, 1), pick(t, v, v, q, p, p).clamp(0, 1),
            pick(p, p, t, v, v, q).clamp(0, 1))


def color(images, params, swap_rb, dtype):
    """The colour map of RGBDAugmentor on images [N, 3, H, W] (0..255) in `dtype`."""
    x = images.to(dtype)
    if not params.do_color:
        return x
    ir, ib = (2, 0) if swap_rb else (0, 2)
    r, g, b = x[:, ir] / 255.0, x[:, 1] / 255.0, x[:, ib] / 255.0
    for op in params.order:
        if op == 0:
            k = torch.tensor(params.brightness, dtype=torch.float32).to(dtype)
            r, g, b = ((c * k).clamp(0, 1) for c in (r, g, b))
        elif op == 1:
            c_ = torch.tensor(params.contrast, dtype=torch.float32).to(dtype)
            m = _gray(r, g, b).to(torch.float64).mean().to(dtype)
            o = (1.0 - c_) * m
            r, g, b = ((c_ * c + o).clamp(0, 1) for c in (r, g, b))
        elif op == 2:
            s_ = torch.tensor(params.saturation, dtype=torch.float32).to(dtype)
            o = (1.0 - s_) * _gray(r, g, b)
            r, g, b = ((s_ * c + o).clamp(0, 1) for c in (r, g, b))
        else:
            r, g, b = _hue(r, g, b, torch.tensor(params.hue, dtype=torch.float32).to(dtype))
    if params.gray:
        r = g = b = _gray(r, g, b)
    if params.invert:
        r, g, b = 1.0 - r, 1.0 - g, 1.0 - b
    planes = [None, g * 255.0, None]
    planes[ir], planes[ib] = r * 255.0, b * 255.0
    return torch.stack(planes, 1)


def spatial(images, disps, intrinsics, scale, crop):
    """augmentation.py:24-57 on the CPU: F.interpolate, then the slice."""
    H, W = images.shape[2:]
    ht1, wd1 = int(scale * H), int(scale * W)
    y0, x0 = (ht1 - crop[0]) // 2, (wd1 - crop[1]) // 2
    K = torch.tensor(scale, dtype=torch.float32) * intrinsics
    K = K - torch.tensor([0.0, 0.0, x0, y0], dtype=torch.float32)
    if scale != 1:
        images = F.interpolate(images, (ht1, wd1), mode="bicubic", align_corners=False)
        disps = F.interpolate(disps[:, None], (ht1, wd1))[:, 0]
    return (images[:, :, y0:y0 + crop[0], x0:x0 + crop[1]],
            disps[:, y0:y0 + crop[0], x0:x0 + crop[1]], K)


# ---- a synthetic TartanAir tree ---------------------------------------------------------
def write_tartan_tree(root, scenes=("envA/envA/Easy/P000", "envB/envB/Hard/P001"), frames=8, H=32,
                      W=48, seed=0):
    """Two scenes of `frames` frames: PIL PNGs, .npy depths, pose_left.txt.  Returns
    {scene path: (images uint8 [n, H, W, 3] RGB, depths [n, H, W], pose file rows)}."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    out = {}
    for s, name in enumerate(scenes):
        d = os.path.join(str(root), name)
        os.makedirs(os.path.join(d, "image_left"))
        os.makedirs(os.path.join(d, "depth_left"))
        imgs = rng.integers(0, 256, (frames, H, W, 3), dtype=np.uint8)
        deps = rng.uniform(5.0, 20.0, (frames, H, W)).astype(np.float32)
        rows = np.zeros((frames, 7))
        rows[:, :3] = np.cumsum(rng.normal(0, 0.05, (frames, 3)), 0) + s
        q = np.concatenate([rng.normal(0, 0.01, (frames, 3)), np.ones((frames, 1))], 1)
        rows[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
        for i in range(frames):
            Image.fromarray(imgs[i]).save(os.path.join(d, "image_left", f"{i:06d}_left.png"))
            np.save(os.path.join(d, "depth_left", f"{i:06d}_left_depth.npy"), deps[i])
        np.savetxt(os.path.join(d, "pose_left.txt"), rows, delimiter=" ")
        out[d] = (imgs, deps, rows)
    return out
