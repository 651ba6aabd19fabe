"""CPU: the C ABI of the feature encoder (include/dpvo_hot.h, dpvo_encoder_*):
status rules without a device, size functions, and the packed weight blob
unpacked by the layout documented in csrc/encoder.hip."""
import ctypes

import numpy as np
import pytest

import encoder_ref

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, F16 = 0, 1
NONE, INSTANCE = 0, 1
NCHW, NHWC = 0, 1
HDR = 256


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    lib.dpvo_encoder_packed_bytes.restype = ctypes.c_size_t
    lib.dpvo_encoder_workspace_bytes.restype = ctypes.c_size_t
    return lib


def pack(lib, P, out_dim, wdtype, norm=INSTANCE, ntensors=22, blob_bytes=None):
    arrs = [np.ascontiguousarray(P[n], np.float32) for n, _ in encoder_ref.param_shapes(out_dim)]
    ptrs = (ctypes.c_void_p * 22)(*[a.ctypes.data for a in arrs])
    n = lib.dpvo_encoder_packed_bytes(out_dim, wdtype) if blob_bytes is None else blob_bytes
    blob = np.full(max(n, 1), 0xAB, np.uint8)
    st = lib.dpvo_encoder_pack_weights(ptrs, ntensors, out_dim, norm, wdtype,
                                       ctypes.c_void_p(blob.ctypes.data), ctypes.c_size_t(n))
    return st, blob


def kpad(cin, k):
    return 160 if cin == 3 else cin * k * k


def unpack_conv(blob, off, cout, Kpad, wdtype):
    """[cout, Kpad] from the packed units: element (n, k) at 16-B unit
    ((n / 16) KS + k / KK) 64 + 16 ((k % KK) / KQ) + n % 16, slot k % KQ."""
    KK, dt = (32, np.float16) if wdtype == F16 else (16, np.float32)
    KQ, KS = KK // 4, Kpad // KK
    flat = blob[off:off + cout * Kpad * np.dtype(dt).itemsize].view(dt)
    n, k = np.meshgrid(np.arange(cout), np.arange(Kpad), indexing="ij")
    unit = ((n // 16) * KS + k // KK) * 64 + 16 * ((k % KK) // KQ) + n % 16
    return flat[unit * KQ + k % KQ]


def test_sizes(lib):
    pb, wb = lib.dpvo_encoder_packed_bytes, lib.dpvo_encoder_workspace_bytes
    assert 0 < pb(128, F16) < pb(384, F16) < pb(384, F32) and pb(128, F16) < pb(128, F32)
    nw = sum(co * kpad(ci, k) for co, ci, k in encoder_ref.conv_shapes(128))
    nb = sum(co for co, _, _ in encoder_ref.conv_shapes(128))
    assert pb(128, F16) == (HDR + 2 * nw + 4 * nb + 255) // 256 * 256
    assert pb(128, F32) == (HDR + 4 * nw + 4 * nb + 255) // 256 * 256
    for bad in (0, -64, 100, 32, 2048):
        assert pb(bad, F16) == 0
    assert pb(128, 2) == 0 and pb(128, 7) == 0
    assert 0 < wb(1, 9, 11, 128) < wb(1, 30, 46, 128) < wb(2, 30, 46, 128) < wb(1, 480, 640, 128)
    assert wb(1, 480, 640, 128) == wb(1, 480, 640, 384)  # the output is the caller's
    # at least the three half-resolution and three quarter-resolution planes
    assert wb(1, 480, 640, 128) >= 3 * 240 * 320 * 32 * 4 + 3 * 120 * 160 * 64 * 4
    assert wb(0, 30, 46, 128) == 0 and wb(1, 0, 46, 128) == 0 and wb(1, 30, -1, 128) == 0
    assert wb(1, 30, 46, 100) == 0


def test_forward_status_rules_without_a_device(lib):
    f = lib.dpvo_encoder_forward
    one = ctypes.c_void_p(64)
    big = ctypes.c_size_t(1 << 40)

    def call(wd=F16, norm=INSTANCE, od=128, n=1, H=30, W=46, layout=NCHW, ws_bytes=big, **null):
        p = {k: one for k in ("blob", "images", "out", "ws")}
        p.update({k: None for k in null})
        return f(p["blob"], wd, norm, od, p["images"], n, H, W, p["out"], layout, p["ws"], ws_bytes,
                 None)

    for name in ("blob", "images", "out", "ws"):
        assert call(**{name: 1}) == INVALID, name
    assert call(n=0) == INVALID and call(n=-2) == INVALID
    assert call(H=0) == INVALID and call(W=0) == INVALID and call(H=-5) == INVALID
    assert call(layout=2) == INVALID
    assert call(wd=2) == UNSUPPORTED and call(wd=5) == UNSUPPORTED   # fp64 weights
    assert call(od=100) == UNSUPPORTED and call(od=0) == UNSUPPORTED and call(od=4096) == UNSUPPORTED
    assert call(norm=2) == UNSUPPORTED                                # batch / group norms
    need = lib.dpvo_encoder_workspace_bytes(1, 30, 46, 128)
    assert need > 0 and call(ws_bytes=ctypes.c_size_t(need - 1)) == WORKSPACE
    assert call(ws_bytes=ctypes.c_size_t(0), layout=NHWC) == WORKSPACE
    # null pointers come first, then the unsupported checks, then the workspace
    assert call(od=100, images=1, ws_bytes=ctypes.c_size_t(0)) == INVALID
    assert call(od=100, ws_bytes=ctypes.c_size_t(0)) == UNSUPPORTED


def test_pack_status_rules(lib):
    P = encoder_ref.formula_params(128, "instance")
    assert pack(lib, P, 128, F16)[0] == OK
    assert pack(lib, P, 128, F32, norm=NONE)[0] == OK
    assert pack(lib, P, 128, F16, ntensors=21)[0] == INVALID
    assert pack(lib, P, 128, F16, ntensors=50)[0] == INVALID
    assert pack(lib, P, 128, 2, blob_bytes=1 << 20)[0] == UNSUPPORTED
    assert pack(lib, P, 128, F16, norm=3)[0] == UNSUPPORTED
    P100 = dict(P)
    assert pack(lib, P100, 128, F16, blob_bytes=lib.dpvo_encoder_packed_bytes(128, F16) - 1)[0] == WORKSPACE
    ptrs = (ctypes.c_void_p * 22)()
    buf = np.zeros(lib.dpvo_encoder_packed_bytes(128, F16), np.uint8)
    assert lib.dpvo_encoder_pack_weights(ptrs, 22, 128, INSTANCE, F16,
                                         ctypes.c_void_p(buf.ctypes.data),
                                         ctypes.c_size_t(buf.size)) == INVALID  # null tensors
    assert lib.dpvo_encoder_pack_weights(None, 22, 128, INSTANCE, F16,
                                         ctypes.c_void_p(buf.ctypes.data),
                                         ctypes.c_size_t(buf.size)) == INVALID
    arrs = [np.ascontiguousarray(P[n], np.float32) for n, _ in encoder_ref.param_shapes(128)]
    ptrs = (ctypes.c_void_p * 22)(*[a.ctypes.data for a in arrs])
    assert lib.dpvo_encoder_pack_weights(ptrs, 22, 96, INSTANCE, F16,
                                         ctypes.c_void_p(buf.ctypes.data),
                                         ctypes.c_size_t(buf.size)) == UNSUPPORTED  # output dim
    assert lib.dpvo_encoder_pack_weights(ptrs, 22, 128, INSTANCE, F16, None,
                                         ctypes.c_size_t(buf.size)) == INVALID


@pytest.mark.parametrize("out_dim,norm", [(128, INSTANCE), (384, NONE)])
@pytest.mark.parametrize("wdtype", [F32, F16])
def test_blob_holds_every_weight(lib, out_dim, norm, wdtype):
    P = encoder_ref.formula_params(out_dim, "instance" if norm == INSTANCE else "none")
    st, blob = pack(lib, P, out_dim, wdtype, norm=norm)
    assert st == OK
    hdr = blob[:16].view(np.int32)
    assert bytes(blob[:4]) == b"ENC1" and list(hdr[1:4]) == [wdtype, out_dim, norm]
    assert not blob[16:HDR].any()
    es = 2 if wdtype == F16 else 4
    wt = np.float16 if wdtype == F16 else np.float32
    off = HDR
    for name, (co, ci, k) in zip(encoder_ref.CONVS, encoder_ref.conv_shapes(out_dim)):
        K, Kp = ci * k * k, kpad(ci, k)
        W = unpack_conv(blob, off, co, Kp, wdtype)
        # K order: tap-major (ky, kx), channel inside
        want = P[name + ".weight"].transpose(0, 2, 3, 1).reshape(co, K).astype(wt)
        assert np.array_equal(W[:, :K], want), name
        assert not W[:, K:].any(), name + ": padded K tail must be zero"
        off += co * Kp * es
    for name, (co, _, _) in zip(encoder_ref.CONVS, encoder_ref.conv_shapes(out_dim)):
        assert np.array_equal(blob[off:off + 4 * co].view(np.float32), P[name + ".bias"]), name
        off += 4 * co
    assert off <= blob.size == lib.dpvo_encoder_packed_bytes(out_dim, wdtype)
    assert not blob[off:].any()
