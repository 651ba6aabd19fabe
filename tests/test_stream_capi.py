"""CPU: host-side validation of dpvo_frame_prepare / dpvo_frame_prepare_shape of
the C ABI, before any launch -- no GPU needed."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED = 0, 1, 3
ONE = ctypes.c_void_p(16)  # non-null, 4-byte aligned, never dereferenced on the host
EUROC = (458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.dpvo_frame_prepare.argtypes = [vp, i, i, i, ctypes.POINTER(d), i, d, i, vp, vp, vp]
    lib.dpvo_frame_prepare_shape.argtypes = [i, i, d, ctypes.POINTER(i), ctypes.POINTER(i)]
    return lib


def _prepare(lib, raw=ONE, H0=480, W0=752, channels=1, calib=EUROC, ncalib=None, scale=1.0,
             swap_rb=0, image=ONE, intrinsics=ONE):
    arr = None if calib is None else (ctypes.c_double * max(len(calib), 1))(*calib)
    n = (0 if calib is None else len(calib)) if ncalib is None else ncalib
    return lib.dpvo_frame_prepare(raw, H0, W0, channels, arr, n, scale, swap_rb, image, intrinsics,
                                  None)


def test_null_pointers(lib):
    assert _prepare(lib, raw=None) == INVALID
    assert _prepare(lib, calib=None, ncalib=8) == INVALID
    assert _prepare(lib, image=None) == INVALID
    assert _prepare(lib, intrinsics=None) == INVALID


def test_bad_sizes_and_flags(lib):
    assert _prepare(lib, H0=0) == INVALID
    assert _prepare(lib, W0=-752) == INVALID
    assert _prepare(lib, channels=2) == INVALID
    assert _prepare(lib, channels=4) == INVALID
    assert _prepare(lib, swap_rb=2) == INVALID
    assert _prepare(lib, image=ctypes.c_void_p(18)) == INVALID  # 32-bit stores


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("bad", [0.0, float("inf"), float("-inf"), float("nan")])
def test_focal_length_zero_or_not_finite(lib, k, bad):
    calib = list(EUROC)
    calib[k] = bad
    assert _prepare(lib, calib=calib) == INVALID
    assert _prepare(lib, calib=calib[:4]) == INVALID


def test_invalid_comes_before_unsupported(lib):
    assert _prepare(lib, H0=0, scale=0.25) == INVALID
    assert _prepare(lib, raw=None, calib=EUROC[:5]) == INVALID


@pytest.mark.parametrize("count", [1, 2, 3, 5, 6, 7, 10, 12])
def test_coefficient_count(lib, count):
    assert _prepare(lib, calib=(EUROC + (0.0,) * 4)[:count]) == UNSUPPORTED


def test_scale_and_odd_sizes(lib):
    assert _prepare(lib, scale=0.25) == UNSUPPORTED
    assert _prepare(lib, scale=2.0) == UNSUPPORTED
    assert _prepare(lib, H0=481, scale=0.5) == UNSUPPORTED
    assert _prepare(lib, W0=753, scale=0.5) == UNSUPPORTED
    assert _prepare(lib, H0=20000) == UNSUPPORTED


def test_empty_output(lib):
    assert _prepare(lib, H0=15) == UNSUPPORTED
    assert _prepare(lib, W0=15) == UNSUPPORTED
    assert _prepare(lib, H0=30, scale=0.5) == UNSUPPORTED


def test_shape(lib):
    H, W = ctypes.c_int(), ctypes.c_int()
    for (h0, w0, scale), want in {(480, 752, 1.0): (480, 752), (50, 84, 1.0): (48, 80),
                                  (1080, 1920, 0.5): (528, 960), (64, 96, 0.5): (32, 48),
                                  (481, 753, 1.0): (480, 752)}.items():
        assert lib.dpvo_frame_prepare_shape(h0, w0, scale, ctypes.byref(H), ctypes.byref(W)) == OK
        assert (H.value, W.value) == want
    assert lib.dpvo_frame_prepare_shape(0, 5, 1.0, ctypes.byref(H), ctypes.byref(W)) == INVALID
    assert lib.dpvo_frame_prepare_shape(64, 96, 1.0, None, ctypes.byref(W)) == INVALID
    assert lib.dpvo_frame_prepare_shape(63, 96, 0.5, ctypes.byref(H), ctypes.byref(W)) == UNSUPPORTED


def test_cpu_tensors_are_rejected_loudly():
    import torch

    import dpvo_amd
    from dpvo_amd import stream

    ext = dpvo_amd.load_extension("cuda_ba")
    assert hasattr(ext, "frame_prepare")
    raw = torch.zeros(32, 48, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        stream.prepare_frame(raw, EUROC)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.frame_prepare(raw, list(EUROC), 1.0, False, None)
    assert dpvo_amd.prepare_frame is stream.prepare_frame
    assert dpvo_amd.ImageStream is stream.ImageStream and dpvo_amd.read_calib is stream.read_calib
