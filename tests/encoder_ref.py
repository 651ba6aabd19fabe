"""fp64 restatement of DPVO's feature encoder (BasicEncoder4) and of the
Patchifier gathers, written from their formulas:

    x   = relu(norm(conv7x7_s2(img)))                          3 -> 32
    block(x, s): y = relu(norm(conv3x3_s(x))); y = relu(norm(conv3x3(y)))
                 out = relu(skip(x) + y),  skip = norm(conv1x1_s(x)) when s = 2
    x   = block(block(x, 1), 1);  x = block(block(x, 2), 1)    32 -> 32 -> 64
    out = conv1x1(x) / 4                                       64 -> out_dim

norm is the identity ('none') or, per image and channel over the plane,
(x - mean) / sqrt(biased var + 1e-5) ('instance').  The / 4 is Patchifier's
(fmap = fnet(images) / 4).  Runs on whatever device its inputs are on, in
float64.  With ``f16_operand=True`` the input activation and the weights of
every convolution are rounded to fp16 (nearest even) and nothing else
changes: the rounding model of the fp16 kernels.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

CONVS = ["conv1", "layer1.0.conv1", "layer1.0.conv2", "layer1.1.conv1", "layer1.1.conv2",
         "layer2.0.conv1", "layer2.0.conv2", "layer2.0.downsample.0", "layer2.1.conv1",
         "layer2.1.conv2", "conv2"]


def conv_shapes(out_dim):
    """(cout, cin, k) of the eleven convolutions in state_dict order."""
    return [(32, 3, 7), (32, 32, 3), (32, 32, 3), (32, 32, 3), (32, 32, 3), (64, 32, 3),
            (64, 64, 3), (64, 32, 1), (64, 64, 3), (64, 64, 3), (out_dim, 64, 1)]


def param_shapes(out_dim):
    out = []
    for name, (co, ci, k) in zip(CONVS, conv_shapes(out_dim)):
        out += [(name + ".weight", (co, ci, k, k)), (name + ".bias", (co,))]
    return out


def out_size(n):
    return (n - 1) // 2 + 1


def _hash01(idx, salt):
    """Closed-form pseudo-noise in [-1, 1): the fractional part of a scaled sine."""
    v = np.sin(idx * 12.9898 + salt * 78.233 + 0.5) * 43758.5453
    return 2.0 * (v - np.floor(v)) - 1.0


def formula_params(out_dim, norm):
    """Deterministic parameters from a closed formula (no RNG), float32 numpy
    arrays keyed by state_dict name.  Weights are uniform-like with the Kaiming
    standard deviation sqrt(2 / fan_in); biases are uniform-like with standard
    deviation 0.1 about 0.02, never zero.  ``norm`` only salts the sequence, so
    fnet and inet differ."""
    salt0 = 100 if norm == "instance" else 200
    out = {}
    for t, (name, shape) in enumerate(param_shapes(out_dim)):
        n = int(np.prod(shape))
        u = _hash01(np.arange(n, dtype=np.float64), salt0 + t + 1).reshape(shape)
        if name.endswith("weight"):
            fan_in = shape[1] * shape[2] * shape[3]
            v = u * math.sqrt(3.0) * math.sqrt(2.0 / fan_in)
        else:
            v = 0.1 * math.sqrt(3.0) * u + 0.02
        out[name] = v.astype(np.float32)
    return out


def to_torch(params, device="cpu"):
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float64, device=device)
            for k, v in params.items()}


def _r16(t):
    return t.to(torch.float16).to(torch.float64)


def encoder_ref(P, images, norm, f16_operand=False):
    """P: dict of float64 tensors (to_torch); images [N, 3, H, W] float64.
    Returns [N, out_dim, h, w] float64, the encoder's output / 4."""
    if norm not in ("instance", "none"):
        raise ValueError(norm)

    def conv(name, x, stride, pad):
        W = P[name + ".weight"]
        if f16_operand:
            x, W = _r16(x), _r16(W)
        return F.conv2d(x, W, P[name + ".bias"], stride=stride, padding=pad)

    def nrm(x):
        if norm == "none":
            return x
        mu = x.mean(dim=(2, 3), keepdim=True)
        var = ((x - mu) ** 2).mean(dim=(2, 3), keepdim=True)
        return (x - mu) / torch.sqrt(var + 1e-5)

    def block(name, x, stride):
        y = torch.relu(nrm(conv(name + ".conv1", x, stride, 1)))
        y = torch.relu(nrm(conv(name + ".conv2", y, 1, 1)))
        if stride != 1:
            x = nrm(conv(name + ".downsample.0", x, stride, 0))
        return torch.relu(x + y)

    x = torch.relu(nrm(conv("conv1", images, 2, 3)))
    x = block("layer1.1", block("layer1.0", x, 1), 1)
    x = block("layer2.1", block("layer2.0", x, 2), 1)
    return conv("conv2", x, 1, 0) / 4.0


def gather_ref(fmap, coords, radius):
    """fmap [n, C, h, w], coords [n, M, 2] integer-valued (x, y): the
    (2 radius + 1)^2 window around each centre -> [n, M, C, D, D]."""
    n, C, h, w = fmap.shape
    M = coords.shape[1]
    D = 2 * radius + 1
    out = torch.zeros(n, M, C, D, D, dtype=fmap.dtype, device=fmap.device)
    for i in range(n):
        for m in range(M):
            x, y = int(coords[i, m, 0]), int(coords[i, m, 1])
            out[i, m] = fmap[i, :, y - radius:y + radius + 1, x - radius:x + radius + 1]
    return out


def patchifier_ref(fmap, imap, images, coords, disps=None, patch_size=3):
    """The Patchifier gathers restated.  fmap [n, 128, h, w], imap
    [n, 384, h, w], images [n, 3, H, W], coords [n, M, 2]; disps [n, h, w] or
    None (ones).  Returns gmap [1, nM, 128, P, P], imap [1, nM, 384, 1, 1],
    patches [1, nM, 3, P, P], index [nM], clr [1, nM, 3]."""
    n, _, h, w = fmap.shape
    M = coords.shape[1]
    R = patch_size // 2
    dt, dev = fmap.dtype, fmap.device
    if disps is None:
        disps = torch.ones(n, h, w, dtype=dt, device=dev)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dt, device=dev),
                            torch.arange(w, dtype=dt, device=dev), indexing="ij")
    grid = torch.stack([xs.expand(n, h, w), ys.expand(n, h, w), disps.to(dt)], dim=1)
    flat = lambda t: t.reshape(1, n * M, *t.shape[2:])
    gmap = flat(gather_ref(fmap, coords, R))
    im = flat(gather_ref(imap, coords, 0))
    patches = flat(gather_ref(grid, coords, R))
    clr = flat(gather_ref(images, 4 * coords + 2, 0)).reshape(1, n * M, 3)
    index = torch.arange(n, device=dev).view(n, 1).repeat(1, M).reshape(-1)
    return gmap, im, patches, index, clr
