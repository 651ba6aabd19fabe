"""CPU: the frame-preparation restatement (stream_ref.py) on its own, and the
host side of dpvo_amd.stream (calibration file, directory listing, decoding)."""
import os

import numpy as np
import pytest

import stream_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _frame(h, w, c=3, seed=0):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (h, w, c) if c else (h, w), dtype=np.uint8)


def test_zero_coefficients_give_the_identity():
    raw = _frame(32, 48)
    for calib in ([40.0, 41.0, 20.3, 15.6, 0, 0, 0, 0], [40.0, 41.0, 20.3, 15.6, 0, 0, 0, 0, 0]):
        r = R.prepare_frame(raw, calib)
        np.testing.assert_array_equal(r["image"], raw.transpose(2, 0, 1))
        assert not r["all_outside"].any()


def test_cx_cancels_without_distortion_and_the_border_reads_zero():
    # the undistorted image keeps the camera matrix, so with zero coefficients cx enters as
    # (u - cx) / fx * fx + cx: the identity map for any cx (exact for these numbers)
    raw = _frame(32, 48, seed=1)
    for cx in (16.0, 19.0, -3.0):
        mx, my = R.distortion_map([32.0, 32.0, cx, 8.0, 0, 0, 0, 0], 32, 48)
        np.testing.assert_array_equal(mx, np.arange(48.0)[None, :] + 0 * my)
        np.testing.assert_array_equal(my, np.arange(32.0)[:, None] + 0 * mx)
    # taps() is the border rule: reading 3 px to the right leaves a zero band on the right
    iy, ix = np.meshgrid(np.arange(32), np.arange(48), indexing="ij")
    val, inside = R.taps(raw, iy, ix + 3)
    np.testing.assert_array_equal(val[:, :45], raw[:, 3:])
    assert not val[:, 45:].any() and not inside[:, 45:].any() and inside[:, :45].all()


def test_integer_shift_gives_the_shifted_image_with_a_zero_border(monkeypatch):
    """A principal point moved by whole pixels between the source and the
    undistorted image, with zero distortion: the map is the identity plus the
    shift (cx alone cancels, above), and undistort() gives the shifted image,
    zero outside."""
    raw = _frame(32, 48, seed=2)
    real = R.distortion_map

    def shifted(calib, h0, w0):
        mx, my = real(calib, h0, w0)
        return mx + 5.0, my - 2.0

    monkeypatch.setattr(R, "distortion_map", shifted)
    r = R.undistort(raw, [32.0, 32.0, 16.0, 8.0, 0, 0, 0, 0])
    want = np.zeros_like(raw)
    want[2:, :43] = raw[:30, 5:]
    np.testing.assert_array_equal(r["image"], want)
    # row 1 blends rows -1 and 0 with weights 32 and 0: a tap inside, the value still 0
    assert r["all_outside"][:1].all() and r["all_outside"][:, 43:].all()
    assert not r["all_outside"][1:, :43].any()


def test_half_pixel_map_is_the_rounded_mean():
    raw = _frame(16, 16, seed=3)
    s = raw.astype(np.int64)
    val = sum(w * R.taps(raw, *np.meshgrid(np.arange(16) + dy, np.arange(16) + dx, indexing="ij"))[0]
              for dy, dx, w in ((0, 0, 256), (0, 1, 256), (1, 0, 256), (1, 1, 256)))
    pad = np.pad(s, ((0, 1), (0, 1), (0, 0)))
    want = (256 * (pad[:-1, :-1] + pad[:-1, 1:] + pad[1:, :-1] + pad[1:, 1:]) + 512) >> 10
    np.testing.assert_array_equal((val + 512) >> 10, want)


def test_halving_a_constant_image_is_constant():
    for value in (0, 1, 77, 255):
        raw = np.full((32, 64, 3), value, np.uint8)
        r = R.prepare_frame(raw, [30.0, 30.0, 32.0, 16.0], scale=0.5)
        assert r["image"].shape == (3, 16, 32)
        assert (r["image"] == value).all()
    np.testing.assert_array_equal(r["intrinsics"], np.float32([15.0, 15.0, 16.0, 8.0]))


def test_halving_rounds_half_up():
    raw = np.zeros((32, 32), np.uint8)
    raw[0, 0], raw[0, 1] = 1, 1   # (1 + 1 + 0 + 0 + 2) >> 2 = 1
    raw[2, 0] = 1                 # (1 + 0 + 0 + 0 + 2) >> 2 = 0
    r = R.prepare_frame(raw, [30.0, 30.0, 16.0, 16.0], scale=0.5)
    assert r["image"][0, 0, 0] == 1 and r["image"][0, 1, 0] == 0
    np.testing.assert_array_equal(r["image"][0], r["image"][1])
    np.testing.assert_array_equal(r["image"][0], r["image"][2])


@pytest.mark.parametrize("h1", [16, 17, 31, 32, 47])
@pytest.mark.parametrize("w1", [16, 17, 31, 32, 47])
def test_crop_sizes(h1, w1):
    want = {16: 16, 17: 16, 31: 16, 32: 32, 47: 32}
    assert R.crop_size(h1, w1) == (want[h1], want[w1])
    r = R.prepare_frame(_frame(h1, w1), [20.0, 20.0, 8.0, 8.0])
    assert r["image"].shape == (3, want[h1], want[w1])
    assert R.output_size(2 * h1, 2 * w1, 0.5) == (want[h1], want[w1])


def test_swap_rb_and_grey():
    raw = _frame(16, 32, seed=4)
    a = R.prepare_frame(raw, [20.0, 20.0, 8.0, 8.0])["image"]
    b = R.prepare_frame(raw, [20.0, 20.0, 8.0, 8.0], swap_rb=True)["image"]
    np.testing.assert_array_equal(a[::-1], b)
    g = R.prepare_frame(raw[..., 0], [20.0, 20.0, 8.0, 8.0], swap_rb=True)["image"]
    for p in range(3):
        np.testing.assert_array_equal(g[p], raw[..., 0])


def test_pincushion_case_has_pixels_with_every_tap_outside():
    import stream_cases as C

    raw = _frame(*C.PINCUSHION["shape"], seed=5)
    r = R.prepare_frame(raw, C.PINCUSHION["calib"])
    H, W = r["image"].shape[1:]
    assert r["all_outside"][:H, :W].any()


def test_stated_map_ranges_of_the_gpu_cases():
    """The issue's figures for the two calibrations: the barrel map stays inside
    the source, the 9-number map reaches -0.94 and 95.49."""
    import stream_cases as C

    mx, my = R.distortion_map(C.BARREL["calib"], *C.BARREL["shape"])
    h, w = C.BARREL["shape"]
    assert mx.min() >= 0 and mx.max() <= w - 1 and my.min() >= 0 and my.max() <= h - 1
    mx, my = R.distortion_map(C.NINE["calib"], *C.NINE["shape"])
    assert round(min(mx.min(), my.min()), 2) == -0.94
    assert round(max(mx.max(), my.max()), 2) == 95.49


# ---- the host side of dpvo_amd.stream ---------------------------------------------------
def test_read_calib_euroc():
    from dpvo_amd.stream import read_calib

    c = read_calib(os.path.join(GOLDEN, "calib_euroc.txt"))
    assert c.dtype == np.float64 and c.shape == (8,)
    np.testing.assert_array_equal(c[:5], [458.654, 457.296, 367.215, 248.375, -0.28340811])


def test_read_calib_refuses_other_counts(tmp_path):
    from dpvo_amd.stream import read_calib

    p = tmp_path / "c.txt"
    p.write_text("1 2 3 4 5")
    with pytest.raises(ValueError, match="4, 8 or 9"):
        read_calib(p)
    p.write_text("500 501 320 240")
    assert read_calib(p).tolist() == [500.0, 501.0, 320.0, 240.0]


@pytest.fixture()
def imagedir(tmp_path):
    from PIL import Image

    names = ["b_%02d.png" % i for i in range(7)] + ["a.jpg", "c.jpeg", "notes.txt", "d.bmp"]
    for k, name in enumerate(names):
        if name.endswith((".txt", ".bmp")):
            (tmp_path / name).write_bytes(b"x")
        elif name.endswith(".png"):
            Image.fromarray(np.full((16, 32), k, np.uint8)).save(tmp_path / name)
        else:
            Image.fromarray(np.full((16, 32, 3), k, np.uint8)).save(tmp_path / name)
    return tmp_path


def test_image_stream_listing_skip_and_stride(imagedir):
    from dpvo_amd.stream import ImageStream, list_images

    every = [p.name for p in list_images(imagedir)]
    assert every == ["a.jpg"] + ["b_%02d.png" % i for i in range(7)] + ["c.jpeg"]
    for skip, stride in ((0, 1), (0, 2), (1, 2), (3, 3), (8, 1), (9, 1), (2, 100)):
        s = ImageStream(imagedir, [20.0, 20.0, 8.0, 8.0], stride=stride, skip=skip)
        assert [p.name for p in s.files] == every[skip::stride]
        assert len(s) == len(every[skip::stride])
    with pytest.raises(FileNotFoundError):
        list_images(imagedir / "missing")


def test_image_stream_decode(imagedir):
    from dpvo_amd.stream import ImageStream

    grey = ImageStream.decode(imagedir / "b_03.png")
    assert grey.dtype == np.uint8 and grey.shape == (16, 32) and (grey == 3).all()
    rgb = ImageStream.decode(imagedir / "a.jpg")
    assert rgb.dtype == np.uint8 and rgb.shape == (16, 32, 3)
