"""GPU: RGBDAugmentor and normalize_depth (csrc/dataset.hip) against the
restatement of tests/dataset_ref.py and torch on the CPU.

Colour / image tolerance: the restatement is run once in fp32 and once in fp64
on the very cases of this file; the tolerance is 4 x the largest gap between
the two runs (values in 0..255), computed in the test from the restatement
alone (`tolerance()`: 1.02e-3 for colour alone, where the hue's division by a
small chroma carries the gap, and 2.40e-3 through the bicubic; the kernels'
largest errors on the MI355X were 2.5e-4 and 5.3e-4).  The colour
map is continuous, so nothing is excluded.  Depth (nearest) and intrinsics
are compared exactly."""
import itertools

import numpy as np
import pytest
import torch

import dataset_ref as ref

pytestmark = pytest.mark.gpu

CROP = (16, 24)


def P(**kw):
    from dpvo_amd.data_readers import AugmentParams

    return AugmentParams(**kw)


def make_images(N=2, H=20, W=28, seed=0):
    """Random frames with exact 0, exact 255 and gray pixels; frame means differ."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 3, H, W, generator=g) * 255.0
    x[:, :, 0, :5] = 0.0
    x[:, :, 1, :5] = 255.0
    x[:, :, 2, :7] = x[:, :1, 2, :7]           # gray: three equal channels
    x[:, 0, 3, :4] = 255.0                      # saturated primaries
    x[:, 1:, 3, :4] = 0.0
    x[:, :, 5, :3] = torch.tensor([10.0, 10.0, 200.0]).view(1, 3, 1)
    if N > 1:
        x[1] = (x[1] * 0.5).clamp(0, 255)       # a darker second frame: another mean
        x[1, :, 1, :5] = 255.0
    return x.contiguous()


def inputs(N=2, H=20, W=28, seed=0):
    g = torch.Generator().manual_seed(seed + 100)
    disps = torch.rand(N, H, W, generator=g) + 0.1
    K = torch.tensor([[30.0, 31.0, 14.2, 9.7]]).repeat(N, 1) + torch.arange(N).view(N, 1) * 0.25
    poses = torch.rand(N, 7, generator=g)
    return make_images(N, H, W, seed), poses, disps, K


J = dict(brightness=1.3, contrast=0.7, saturation=1.35, hue=0.05)
ORDERS = [(1, 0, 2, 3), (1, 3, 2, 0), (0, 1, 3, 2), (3, 2, 1, 0), (2, 0, 3, 1), (0, 3, 2, 1)]
assert {o.index(1) for o in ORDERS} == {0, 1, 2, 3}    # contrast first, in the middle, last
COLOR = {
    "brightness": P(do_color=True, brightness=1.3),
    "brightness_down": P(do_color=True, brightness=0.65),
    "contrast": P(do_color=True, contrast=0.7),
    "contrast_up": P(do_color=True, contrast=1.4),
    "saturation": P(do_color=True, saturation=1.35),
    "saturation_down": P(do_color=True, saturation=0.6),
    "hue": P(do_color=True, hue=0.06),
    "hue_neg": P(do_color=True, hue=-0.2 / 3.14),
    **{"order_" + "".join(map(str, o)): P(do_color=True, order=o, **J) for o in ORDERS},
    "gray": P(do_color=True, gray=True, **J),
    "invert": P(do_color=True, invert=True, **J),
    "gray_invert": P(do_color=True, gray=True, invert=True, order=(2, 1, 0, 3), **J),
}
SCALES = [1.0, 2 ** 0.5, 1.37]
SIZES = [(20, 28), (21, 29)]      # the second makes y0 and x0 odd at scale 1


def restated(images, disps, K, p, swap_rb, dtype):
    c = ref.color(images, p, swap_rb, dtype)
    return ref.spatial(c, disps.to(dtype), K, p.scale, CROP)


_tol = {}


def tolerance(spatial):
    """4 x the largest fp32 / fp64 gap of the restatement over this file's cases."""
    if spatial not in _tol:
        gap = 0.0
        for (H, W), swap in itertools.product(SIZES, (False, True)):
            images, _, disps, K = inputs(2, H, W)
            for p in COLOR.values():
                for s in (SCALES[1:] if spatial else [1.0]):
                    q = P(**{**p.__dict__, "scale": s})
                    a = restated(images, disps, K, q, swap, torch.float32)[0]
                    b = restated(images, disps, K, q, swap, torch.float64)[0]
                    gap = max(gap, float((a.double() - b).abs().max()))
        _tol[spatial] = 4.0 * gap
        print("tolerance", "spatial" if spatial else "colour", _tol[spatial])
    return _tol[spatial]


def run(gpu, images, poses, disps, K, p, swap_rb=False, crop=CROP):
    from dpvo_amd.data_readers import RGBDAugmentor

    aug = RGBDAugmentor(crop, swap_rb=swap_rb)
    out = aug(images.to(gpu), poses.to(gpu), disps.to(gpu), K.to(gpu), params=p)
    return [t.cpu() for t in out]


def check(gpu, images, poses, disps, K, p, swap_rb, tol):
    got_i, got_p, got_d, got_K = run(gpu, images, poses, disps, K, p, swap_rb)
    want_i, want_d, want_K = restated(images, disps, K, p, swap_rb, torch.float64)
    assert got_i.shape == want_i.shape and got_i.dtype == torch.float32
    err = float((got_i.double() - want_i).abs().max())
    print("max err", err, "tol", tol)
    assert err <= tol
    assert torch.equal(got_d, want_d.float())
    assert torch.equal(got_K.view(torch.int32), want_K.view(torch.int32))
    assert torch.equal(got_p, poses)


@pytest.mark.parametrize("swap_rb", [False, True])
@pytest.mark.parametrize("name", list(COLOR))
def test_colour(gpu, name, swap_rb):
    images, poses, disps, K = inputs()
    check(gpu, images, poses, disps, K, COLOR[name], swap_rb, tolerance(False))


def test_swap_rb_says_which_plane_is_red(gpu):
    images, poses, disps, K = inputs()
    p = COLOR["order_3210"]
    a = run(gpu, images, poses, disps, K, p, swap_rb=True)[0]
    b = run(gpu, images.flip(1).contiguous(), poses, disps, K, p, swap_rb=False)[0].flip(1)
    assert torch.equal(a, b)
    c = run(gpu, images, poses, disps, K, p, swap_rb=False)[0]
    assert float((a - c).abs().max()) > 1.0


@pytest.mark.parametrize("size", SIZES)
def test_no_colour_at_scale_one_returns_the_input_bits(gpu, size):
    images, poses, disps, K = inputs(2, *size)
    got_i, _, got_d, got_K = run(gpu, images, poses, disps, K, P(do_color=False, **J, gray=True))
    y0, x0 = (size[0] - CROP[0]) // 2, (size[1] - CROP[1]) // 2
    win = (slice(None), slice(None), slice(y0, y0 + CROP[0]), slice(x0, x0 + CROP[1]))
    assert torch.equal(got_i.view(torch.int32), images[win].contiguous().view(torch.int32))
    assert torch.equal(got_d, disps[win[0], win[2], win[3]])
    assert torch.equal(got_K, K - torch.tensor([0.0, 0.0, x0, y0]))
    # the whole frame as the crop
    full = run(gpu, images, poses, disps, K, P(), crop=size)[0]
    assert torch.equal(full, images)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", [None, "order_1320", "gray_invert"])
def test_spatial(gpu, size, scale, name):
    images, poses, disps, K = inputs(2, *size)
    base = P(do_color=False) if name is None else COLOR[name]
    p = P(**{**base.__dict__, "scale": scale})
    tol = tolerance(scale != 1.0) if (name or scale != 1.0) else 0.0
    check(gpu, images, poses, disps, K, p, True, tol)


def test_spatial_against_interpolate_alone(gpu):
    """No colour: the image is F.interpolate on the CPU followed by the slice."""
    import torch.nn.functional as F

    images, poses, disps, K = inputs(2, 21, 29)
    s = 1.37
    got = run(gpu, images, poses, disps, K, P(scale=s))
    ht1, wd1 = int(s * 21), int(s * 29)
    y0, x0 = (ht1 - 16) // 2, (wd1 - 24) // 2
    want = F.interpolate(images, (ht1, wd1), mode="bicubic", align_corners=False)
    assert float((got[0] - want[:, :, y0:y0 + 16, x0:x0 + 24]).abs().max()) <= tolerance(True)
    wd = F.interpolate(disps[:, None], (ht1, wd1))[:, 0, y0:y0 + 16, x0:x0 + 24]
    assert torch.equal(got[2], wd)
    # not clamped: the bicubic overshoots 0..255 somewhere on random frames
    assert float(got[0].max()) > 255.0 or float(got[0].min()) < 0.0


def test_contrast_mean_pools_the_frames(gpu):
    images, poses, disps, K = inputs()
    p = COLOR["contrast"]
    both = run(gpu, images, poses, disps, K, p)[0]
    alone = [run(gpu, images[i:i + 1], poses[i:i + 1], disps[i:i + 1], K[i:i + 1], p)[0] for i in (0, 1)]
    for i in (0, 1):
        assert float((both[i] - alone[i][0]).abs().max()) > 1.0
    # and the N = 1 results are the restatement's own N = 1 results
    for i in (0, 1):
        want = restated(images[i:i + 1], disps[i:i + 1], K[i:i + 1], p, False, torch.float64)[0]
        assert float((alone[i].double() - want).abs().max()) <= tolerance(False)


def test_two_calls_identical_bits(gpu):
    images, poses, disps, K = inputs(2, 21, 29)
    p = P(**{**COLOR["order_1320"].__dict__, "scale": 1.37})
    a = run(gpu, images, poses, disps, K, p)
    b = run(gpu, images, poses, disps, K, p)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_random_draws(gpu):
    from dpvo_amd.data_readers import AugmentParams

    rng = np.random.default_rng(0)
    draws = [AugmentParams.draw(rng) for _ in range(400)]
    assert 0.4 < np.mean([d.do_color for d in draws]) < 0.6
    assert 0.12 < np.mean([d.scale == 1.0 for d in draws]) < 0.28
    assert all(1.0 <= d.scale <= 2 ** 0.5 and sorted(d.order) == [0, 1, 2, 3] for d in draws)
    assert all(0.6 <= v <= 1.4 for d in draws for v in (d.brightness, d.contrast, d.saturation))
    assert all(abs(d.hue) <= 0.2 / 3.14 for d in draws)
    assert 0.04 < np.mean([d.gray for d in draws]) < 0.17 and len({d.order for d in draws}) == 24
    images, poses, disps, K = inputs()
    a = run(gpu, images, poses, disps, K, AugmentParams.draw(np.random.default_rng(3)))
    b = run(gpu, images, poses, disps, K, AugmentParams.draw(np.random.default_rng(3)))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- normalize_depth -------------------------------------------------------------------------
def depth_cases():
    g = torch.Generator().manual_seed(7)
    rand = torch.rand(2, 16, 24, generator=g) * 3 + 0.01
    few = torch.tensor([0.25, 0.5, 0.5000001, 1.0, 257.0, 1.0000001])[torch.randint(0, 6, (2, 16, 24), generator=g)]
    inf = rand.clone()
    inf.view(-1)[torch.randperm(768, generator=g)[:5]] = float("inf")
    return {"random": rand, "ties": few, "inf": inf}


@pytest.mark.parametrize("name", ["random", "ties", "inf"])
def test_normalize_depth(gpu, name):
    from dpvo_amd.data_readers import normalize_depth

    disps = depth_cases()[name]
    assert disps.numel() == 768
    poses = torch.rand(2, 7, generator=torch.Generator().manual_seed(1)) + 0.5
    d, p, s = (t.cpu() for t in normalize_depth(disps.to(gpu), poses.to(gpu), return_scale=True))
    srt = torch.sort(disps.reshape(-1)).values
    pos = np.float32(0.98) * np.float32(767)
    lo, hi = int(np.floor(pos)), int(np.ceil(pos))
    assert torch.equal(s[1:], torch.stack([srt[lo], srt[hi]]))           # the order statistics, exactly
    want = 0.7 * torch.quantile(disps, 0.98)
    assert torch.isfinite(want) and want > 0
    ulp = np.spacing(np.float32(float(want)))
    assert abs(float(s[0]) - float(want)) <= 2 * ulp
    assert torch.equal(d, disps / s[0]) and d.shape == disps.shape
    wp = poses.clone()
    wp[:, :3] *= s[0]
    assert torch.equal(p, wp)
    d2, p2 = normalize_depth(disps.to(gpu), poses.to(gpu))
    assert torch.equal(d2.cpu(), d) and torch.equal(p2.cpu(), p)


def test_normalize_depth_nan_and_small(gpu):
    from dpvo_amd.data_readers import normalize_depth

    x = torch.rand(300) + 0.1
    x[17] = float("nan")
    _, _, s = normalize_depth(x.to(gpu), torch.rand(1, 7).to(gpu), return_scale=True)
    assert torch.isnan(s).all()                       # torch.quantile's answer
    one = torch.tensor([2.0])
    d, _, s = normalize_depth(one.to(gpu), torch.rand(1, 7).to(gpu), return_scale=True)
    assert float(s[0]) == float(0.7 * torch.quantile(one, 0.98)) and float(s[1]) == 2.0
