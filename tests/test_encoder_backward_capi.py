"""CPU: the C ABI of the encoders' training surface (include/dpvo_hot.h:
dpvo_encoder_saved_bytes, dpvo_encoder_forward_train,
dpvo_encoder_backward_workspace_bytes, dpvo_encoder_backward,
dpvo_encoder_pack_weights_device): size functions and the status rules, all of
which are decided before any launch, so they run without a device."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, F16 = 0, 1
NONE, INSTANCE = 0, 1
NCHW, NHWC = 0, 1


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    lib.dpvo_encoder_saved_bytes.restype = ctypes.c_size_t
    lib.dpvo_encoder_backward_workspace_bytes.restype = ctypes.c_size_t
    lib.dpvo_encoder_workspace_bytes.restype = ctypes.c_size_t
    lib.dpvo_encoder_packed_bytes.restype = ctypes.c_size_t
    return lib


one = ctypes.c_void_p(64)
big = ctypes.c_size_t(1 << 40)


def ptrs22(null_at=None):
    a = (ctypes.c_void_p * 22)(*[64] * 22)
    if null_at is not None:
        a[null_at] = None
    return a


def test_sizes_are_zero_where_the_forward_refuses(lib):
    sb, bw, wb = (lib.dpvo_encoder_saved_bytes, lib.dpvo_encoder_backward_workspace_bytes,
                  lib.dpvo_encoder_workspace_bytes)
    refused = [(0, 30, 46, 128), (1, 0, 46, 128), (1, 30, -1, 128), (1, 30, 46, 100),
               (1, 30, 46, 0), (1, 30, 46, 2048), (70000, 30, 46, 128), (1, 70000 * 2, 46, 128),
               (4, 60000, 60000, 128), (-3, 30, 46, 128)]
    for n, H, W, od in refused:
        assert wb(n, H, W, od) == 0
        assert bw(n, H, W, od) == 0, (n, H, W, od)
        for norm in (NONE, INSTANCE):
            assert sb(n, H, W, od, norm) == 0, (n, H, W, od, norm)
    assert sb(1, 30, 46, 128, 2) == 0 and sb(1, 30, 46, 128, -1) == 0  # other norms
    for norm in (NONE, INSTANCE):
        assert sb(1, 30, 46, 128, norm) > 0
    assert bw(1, 30, 46, 128) > 0


def test_sizes_are_monotone(lib):
    sb, bw = lib.dpvo_encoder_saved_bytes, lib.dpvo_encoder_backward_workspace_bytes
    seq = [(1, 9, 11), (1, 9, 46), (1, 30, 46), (2, 30, 46), (3, 30, 46), (3, 96, 128),
           (3, 480, 640), (15, 480, 640)]
    for norm in (NONE, INSTANCE):
        v = [sb(n, H, W, 128, norm) for n, H, W in seq]
        assert all(a < b for a, b in zip(v, v[1:])), v
    v = [bw(n, H, W, 384) for n, H, W in seq]
    assert all(a < b for a, b in zip(v, v[1:])), v
    # 'instance' keeps the block outputs and the statistics on top of the ten planes
    assert sb(1, 480, 640, 128, INSTANCE) > sb(1, 480, 640, 128, NONE)
    assert sb(1, 480, 640, 128, NONE) >= 5 * 240 * 320 * 32 * 4 + 5 * 120 * 160 * 64 * 4
    assert sb(1, 480, 640, 128, INSTANCE) >= 7 * 240 * 320 * 32 * 4 + 7 * 120 * 160 * 64 * 4
    # the cotangent's channels-last copy is part of the workspace
    assert bw(1, 480, 640, 384) - bw(1, 480, 640, 128) >= 120 * 160 * 256 * 4


def test_forward_train_status_rules_without_a_device(lib):
    f = lib.dpvo_encoder_forward_train

    def call(wd=F32, norm=INSTANCE, od=128, n=1, H=30, W=46, layout=NCHW, sbytes=big, **null):
        p = {k: one for k in ("blob", "images", "out", "saved")}
        p.update({k: None for k in null})
        return f(p["blob"], wd, norm, od, p["images"], n, H, W, p["out"], layout, p["saved"],
                 sbytes, None)

    for name in ("blob", "images", "out", "saved"):
        assert call(**{name: 1}) == INVALID, name
    assert call(n=0) == INVALID and call(H=0) == INVALID and call(W=-1) == INVALID
    assert call(layout=2) == INVALID and call(layout=-1) == INVALID
    assert call(wd=2) == UNSUPPORTED and call(od=100) == UNSUPPORTED and call(norm=2) == UNSUPPORTED
    for norm in (NONE, INSTANCE):
        need = lib.dpvo_encoder_saved_bytes(1, 30, 46, 128, norm)
        assert need > 0
        assert call(norm=norm, sbytes=ctypes.c_size_t(need - 1)) == WORKSPACE
        assert call(norm=norm, sbytes=ctypes.c_size_t(0), layout=NHWC) == WORKSPACE
    assert call(od=100, images=1, sbytes=ctypes.c_size_t(0)) == INVALID
    assert call(od=100, sbytes=ctypes.c_size_t(0)) == UNSUPPORTED


def test_backward_status_rules_without_a_device(lib):
    f = lib.dpvo_encoder_backward

    def call(norm=INSTANCE, od=128, n=1, H=30, W=46, layout=NCHW, wbytes=big, parr=None,
             garr=None, **null):
        p = {k: one for k in ("images", "saved", "grad_out", "ws")}
        p.update({k: None for k in null if k in p})
        pa = None if "params" in null else (parr if parr is not None else ptrs22())
        ga = None if "grads" in null else (garr if garr is not None else ptrs22())
        return f(norm, od, pa, p["images"], n, H, W, p["saved"], p["grad_out"], layout, ga,
                 p["ws"], wbytes, None)

    for name in ("images", "saved", "grad_out", "ws", "params", "grads"):
        assert call(**{name: 1}) == INVALID, name
    for k in (0, 7, 21):
        assert call(parr=ptrs22(k)) == INVALID
        assert call(garr=ptrs22(k)) == INVALID
    assert call(n=0) == INVALID and call(H=0) == INVALID and call(W=-4) == INVALID
    assert call(layout=2) == INVALID and call(layout=-1) == INVALID
    assert call(norm=2) == UNSUPPORTED and call(norm=-1) == UNSUPPORTED
    assert call(od=100) == UNSUPPORTED and call(od=0) == UNSUPPORTED and call(od=4096) == UNSUPPORTED
    for od in (128, 384):
        need = lib.dpvo_encoder_backward_workspace_bytes(1, 30, 46, od)
        assert need > 0
        assert call(od=od, wbytes=ctypes.c_size_t(need - 1)) == WORKSPACE
        assert call(od=od, norm=NONE, wbytes=ctypes.c_size_t(0), layout=NHWC) == WORKSPACE
    # null pointers come first, then the unsupported checks, then the workspace
    assert call(od=100, saved=1, wbytes=ctypes.c_size_t(0)) == INVALID
    assert call(od=100, wbytes=ctypes.c_size_t(0)) == UNSUPPORTED


def test_pack_weights_device_status_rules_without_a_device(lib):
    f = lib.dpvo_encoder_pack_weights_device

    def call(params="ok", od=128, norm=INSTANCE, wd=F32, blob=one, nbytes=big):
        return f(ptrs22() if params == "ok" else params, od, norm, wd, blob, nbytes, None)

    assert call(params=None) == INVALID and call(blob=None) == INVALID
    for k in (0, 10, 21):
        assert call(params=ptrs22(k)) == INVALID
    assert call(od=96) == UNSUPPORTED and call(od=0) == UNSUPPORTED
    assert call(norm=3) == UNSUPPORTED and call(wd=2) == UNSUPPORTED and call(wd=-1) == UNSUPPORTED
    for wd in (F32, F16):
        need = lib.dpvo_encoder_packed_bytes(384, wd)
        assert call(od=384, wd=wd, nbytes=ctypes.c_size_t(need - 1)) == WORKSPACE
    assert call(od=96, blob=None, nbytes=ctypes.c_size_t(0)) == INVALID
    assert call(od=96, nbytes=ctypes.c_size_t(0)) == UNSUPPORTED
