"""GPU: frame_prepare (dpvo_amd/csrc/stream.hip, dpvo_amd.stream.prepare_frame)
against the numpy restatement of tests/stream_ref.py, bit for bit.

The map is fp64 with FMA contraction off on the device and plain numpy on the
host, so both round every operation once, in the same order; what follows the
floor is integer arithmetic.  A pixel may be left out of the comparison only
where the restatement's map * 32 + 0.5 lies within 1e-6 of an integer (there a
last-bit difference of a host and a device division could flip the floor); the
excluded share is capped at 0.1 % per case and the cap is asserted.  On the
cases below the restatement excludes nothing, and on an MI355X every byte of
every case matched."""
import os

import numpy as np
import pytest
import torch

import stream_cases as C
import stream_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_REF = {}

# name -> (case, channels, scale, swap_rb)
CASES = {
    "barrel8": (C.BARREL, 3, 1.0, False),
    "nine": (C.NINE, 3, 1.0, False),
    "pincushion": (C.PINCUSHION, 3, 1.0, False),
    "plain4": (C.PLAIN, 3, 1.0, False),
    "grey": (C.BARREL, 1, 1.0, False),
    "grey_plain4": (C.PLAIN, 1, 1.0, True),
    "swap_rb": (C.NINE, 3, 1.0, True),
    "swap_rb_plain4": (C.PLAIN, 3, 1.0, True),
    "half": (C.NINE, 3, 0.5, False),
    "half_grey": (C.NINE, 1, 0.5, False),
    "half_plain4": (dict(shape=(64, 96), calib=C.PLAIN["calib"]), 3, 0.5, True),
    "half_pincushion": (dict(shape=(64, 104), calib=C.PINCUSHION["calib"]), 1, 0.5, False),
}


def reference(name):
    """(raw, the restatement's result), computed once per case."""
    if name not in _REF:
        case, ch, scale, swap = CASES[name]
        g = np.random.default_rng(sorted(CASES).index(name))
        h, w = case["shape"]
        raw = g.integers(0, 256, (h, w, 3) if ch == 3 else (h, w), dtype=np.uint8)
        _REF[name] = (raw, R.prepare_frame(raw, case["calib"], scale, swap))
    return _REF[name]


def compare(image, intrinsics, ref):
    assert image.dtype == torch.uint8 and intrinsics.dtype == torch.float32
    got = image.cpu().numpy()
    assert got.shape == ref["image"].shape
    np.testing.assert_array_equal(intrinsics.cpu().numpy().view(np.uint32),
                                  ref["intrinsics"].view(np.uint32))
    excluded = ref["margin"] < C.MARGIN
    share = excluded.mean()
    assert share <= C.MAX_EXCLUDED, share
    diff = (got != ref["image"]) & ~excluded[None]
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())
    return share


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement(gpu, name):
    from dpvo_amd.stream import prepare_frame

    case, ch, scale, swap = CASES[name]
    raw, ref = reference(name)
    if "pincushion" in name:  # asserted on the restatement before comparing
        H1, W1 = ref["margin"].shape
        k = 2 if scale == 0.5 else 1
        assert ref["all_outside"][:k * H1, :k * W1].any()
    image, intrinsics = prepare_frame(torch.from_numpy(raw).to(gpu), case["calib"], scale, swap)
    assert tuple(image.shape) == (3,) + R.output_size(*case["shape"], scale)
    assert image.is_contiguous()
    share = compare(image, intrinsics, ref)
    print(f"{name}: excluded share {share:.2e}")


def test_euroc_calibration_at_a_cropped_size(gpu):
    """EuRoC's own line at a quarter-size frame around the principal point's
    scale: the strong barrel coefficients at the focal length they belong to."""
    from dpvo_amd.stream import prepare_frame, read_calib

    calib = read_calib(os.path.join(GOLDEN, "calib_euroc.txt"))
    calib[:4] /= 4  # 120 x 188 frame
    raw = np.random.default_rng(40).integers(0, 256, (120, 188), dtype=np.uint8)
    ref = R.prepare_frame(raw, calib)
    image, intrinsics = prepare_frame(torch.from_numpy(raw).to(gpu), calib)
    assert tuple(image.shape) == (3, 112, 176)
    compare(image, intrinsics, ref)


def test_out_buffer_is_written_in_place(gpu):
    from dpvo_amd.stream import prepare_frame

    raw, ref = reference("barrel8")
    out = torch.full((3, 48, 80), 7, dtype=torch.uint8, device=gpu)
    image, intrinsics = prepare_frame(torch.from_numpy(raw).to(gpu), C.BARREL["calib"], out=out)
    assert image.data_ptr() == out.data_ptr()
    compare(out, intrinsics, ref)
    raw2, ref2 = reference("pincushion")  # the same buffer again: nothing of the first call is left
    _, intrinsics2 = prepare_frame(torch.from_numpy(raw2).to(gpu), C.PINCUSHION["calib"], out=out)
    compare(out, intrinsics2, ref2)
    for bad in (torch.zeros(3, 48, 96, dtype=torch.uint8, device=gpu),
                torch.zeros(3, 48, 80, dtype=torch.float32, device=gpu),
                torch.zeros(3, 48, 160, dtype=torch.uint8, device=gpu)[:, :, ::2]):
        with pytest.raises(RuntimeError, match="out must be"):
            prepare_frame(torch.from_numpy(raw).to(gpu), C.BARREL["calib"], out=bad)


def test_two_calls_are_bit_identical(gpu):
    from dpvo_amd.stream import prepare_frame

    for name in ("nine", "half"):
        case, ch, scale, swap = CASES[name]
        raw = torch.from_numpy(reference(name)[0]).to(gpu)
        a = prepare_frame(raw, case["calib"], scale, swap)
        b = prepare_frame(raw, case["calib"], scale, swap)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_non_contiguous_raw_and_refusals(gpu):
    from dpvo_amd.stream import prepare_frame

    raw, ref = reference("barrel8")
    wide = torch.zeros(50, 100, 3, dtype=torch.uint8, device=gpu)
    wide[:, :84] = torch.from_numpy(raw).to(gpu)
    compare(*prepare_frame(wide[:, :84], C.BARREL["calib"]), ref)
    d = torch.from_numpy(raw).to(gpu)
    with pytest.raises(RuntimeError, match="uint8"):
        prepare_frame(d.float(), C.BARREL["calib"])
    with pytest.raises(RuntimeError, match="unsupported|UNSUPPORTED|status 3"):
        prepare_frame(d, C.BARREL["calib"][:5])
    with pytest.raises(RuntimeError, match="unsupported|UNSUPPORTED|status 3"):
        prepare_frame(d[:, :83], C.BARREL["calib"], scale=0.5)
    with pytest.raises(RuntimeError, match="status 1|invalid|INVALID"):
        prepare_frame(d, (0.0,) + tuple(C.BARREL["calib"][1:]))


def test_prepared_frame_goes_into_the_tracker(gpu):
    """A raw 70 x 100 frame -> [3, 64, 96], the size the tracker tests run at
    with a randomly initialised VONet: one DPVO.__call__ takes it as it is."""
    from dpvo_amd import DPVO, VONet, default_config
    from dpvo_amd.stream import prepare_frame

    cfg = default_config()
    cfg.PATCHES_PER_FRAME, cfg.PATCH_LIFETIME, cfg.REMOVAL_WINDOW = 8, 3, 5
    cfg.OPTIMIZATION_WINDOW, cfg.BUFFER_SIZE, cfg.MAX_EDGES = 4, 64, 2000
    torch.manual_seed(5)
    net = VONet(dtype=torch.float16)
    raw = torch.randint(0, 256, (70, 100, 3), generator=torch.Generator().manual_seed(6),
                        dtype=torch.uint8).to(gpu)
    image, intrinsics = prepare_frame(raw, (320.0, 320.0, 48.0, 32.0, -0.05, 0.01, 0.0, 0.0))
    assert image.dtype == torch.uint8 and tuple(image.shape) == (3, 64, 96)
    assert intrinsics.dtype == torch.float32 and tuple(intrinsics.shape) == (4,)
    slam = DPVO(cfg, net, ht=64, wd=96, device=gpu,
                generator=torch.Generator(device=gpu).manual_seed(8))
    slam(0.0, image, intrinsics)
    assert slam.n == 1
    assert torch.equal(slam.intrinsics_[0].cpu(), intrinsics.cpu() / 4)
