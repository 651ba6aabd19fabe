"""CPU: the C ABI of the update operator (include/dpvo_hot.h, dpvo_update_*):
status rules without a device, size functions, and the packed weight blob
unpacked by the layout documented in csrc/update_op.hip."""
import ctypes

import numpy as np
import pytest

import update_ref

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, F16 = 0, 1
DIM = 384
HDR = 256

# GEMM layers and LayerNorms in blob order
LAYERS = ["corr.0", "corr.2", "corr.5", "c1.0", "c1.2", "c2.0", "c2.2", "agg_kk.f", "agg_kk.g",
          "agg_kk.h", "agg_ij.f", "agg_ij.g", "agg_ij.h", "gru.1.gate.0", "gru.1.res.0",
          "gru.1.res.2", "gru.3.gate.0", "gru.3.res.0", "gru.3.res.2"]
NORMS = ["norm", "corr.3", "gru.0", "gru.2"]


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    lib.dpvo_update_packed_bytes.restype = ctypes.c_size_t
    lib.dpvo_update_workspace_bytes.restype = ctypes.c_size_t
    return lib


def pack(lib, P, K0, wdtype, dim=DIM, ntensors=50, blob_bytes=None):
    arrs = [np.ascontiguousarray(P[n], np.float32) for n, _ in update_ref.param_shapes(K0)]
    ptrs = (ctypes.c_void_p * 50)(*[a.ctypes.data for a in arrs])
    n = lib.dpvo_update_packed_bytes(K0, wdtype) if blob_bytes is None else blob_bytes
    blob = np.full(max(n, 1), 0xAB, np.uint8)
    st = lib.dpvo_update_pack_weights(ptrs, ntensors, dim, K0, wdtype,
                                      ctypes.c_void_p(blob.ctypes.data), ctypes.c_size_t(n))
    return st, blob


def unpack_layer(blob, off, K, Kpad, wdtype):
    """[384, Kpad] from the packed units: element (n, k) at 16-B unit
    ((n / 16) KS + k / KK) 64 + 16 ((k % KK) / KQ) + n % 16, slot k % KQ."""
    KK, dt = (32, np.float16) if wdtype == F16 else (16, np.float32)
    KQ, KS = KK // 4, Kpad // KK
    flat = blob[off:off + DIM * Kpad * np.dtype(dt).itemsize].view(dt)
    n, k = np.meshgrid(np.arange(DIM), np.arange(Kpad), indexing="ij")
    unit = ((n // 16) * KS + k // KK) * 64 + 16 * ((k % KK) // KQ) + n % 16
    return flat[unit * KQ + k % KQ]


def test_sizes_grow(lib):
    pb, wb = lib.dpvo_update_packed_bytes, lib.dpvo_update_workspace_bytes
    assert pb(49, F16) < pb(882, F16) < pb(882, F32) and pb(49, F32) < pb(882, F32)
    assert pb(882, F16) >= 2 * DIM * (896 + 18 * DIM)
    assert pb(0, F16) == 0 and pb(882, 2) == 0 and pb(882, 7) == 0
    assert 0 < wb(1, 882) < wb(48, 882) < wb(2048, 882) < wb(9850, 882)
    assert wb(2048, 49) <= wb(2048, 882)
    assert wb(9850, 882) >= 4 * 9850 * DIM * 4  # f, g, the second x, the group rows
    assert wb(0, 882) == 0 and wb(16, 0) == 0


def test_forward_status_rules_without_a_device(lib):
    f = lib.dpvo_update_forward
    one = ctypes.c_void_p(64)
    big = ctypes.c_size_t(1 << 40)

    def call(wd=F16, E=16, dim=DIM, K0=882, io=F32, ws_bytes=big, **null):
        p = {k: one for k in ("blob", "net", "inp", "corr", "ix", "jx", "ws", "out", "d", "w")}
        p.update({k: None for k in null})
        return f(p["blob"], wd, p["net"], p["inp"], p["corr"], p["ix"], p["jx"], E, dim, K0, io,
                 p["ws"], ws_bytes, p["out"], p["d"], p["w"], None)

    assert call(E=0) == OK and call(E=-3) == OK  # no launch, pointers never read
    assert call(E=0, blob=1, net=1, ws=1) == OK
    assert call(dim=512) == UNSUPPORTED and call(dim=383) == UNSUPPORTED
    assert call(wd=2) == UNSUPPORTED                 # fp64 weights
    assert call(wd=F32, io=F16) == UNSUPPORTED       # fp16 I/O needs fp16 weights
    assert call(io=2) == UNSUPPORTED
    assert call(K0=0) == INVALID
    for name in ("blob", "net", "inp", "corr", "ix", "jx", "ws", "out", "d", "w"):
        assert call(**{name: 1}) == INVALID, name
    need = lib.dpvo_update_workspace_bytes(16, 882)
    assert call(ws_bytes=ctypes.c_size_t(need - 1)) == WORKSPACE
    # the unsupported checks come first, then null pointers, then the workspace
    assert call(dim=512, net=1, ws_bytes=ctypes.c_size_t(0)) == UNSUPPORTED
    assert call(net=1, ws_bytes=ctypes.c_size_t(0)) == INVALID


def test_plan_status_rules_without_a_device(lib):
    f = lib.dpvo_update_plan
    one = ctypes.c_void_p(64)
    assert f(None, None, 0, None, ctypes.c_size_t(0), None) == OK
    assert f(None, one, 8, one, ctypes.c_size_t(1 << 30), None) == INVALID
    assert f(one, None, 8, one, ctypes.c_size_t(1 << 30), None) == INVALID
    assert f(one, one, 8, None, ctypes.c_size_t(1 << 30), None) == INVALID
    need = lib.dpvo_update_workspace_bytes(8, 882)
    assert f(one, one, 8, one, ctypes.c_size_t(need - 1), None) == WORKSPACE


def test_pack_status_rules(lib):
    P = update_ref.formula_params(49)
    assert pack(lib, P, 49, F16)[0] == OK
    assert pack(lib, P, 49, F16, dim=256)[0] == UNSUPPORTED
    assert pack(lib, P, 49, 2, blob_bytes=1 << 20)[0] == UNSUPPORTED
    assert pack(lib, P, 49, F16, ntensors=49)[0] == INVALID
    assert pack(lib, P, 49, F16, blob_bytes=lib.dpvo_update_packed_bytes(49, F16) - 1)[0] == WORKSPACE
    ptrs = (ctypes.c_void_p * 50)()
    buf = np.zeros(lib.dpvo_update_packed_bytes(49, F16), np.uint8)
    assert lib.dpvo_update_pack_weights(ptrs, 50, DIM, 49, F16, ctypes.c_void_p(buf.ctypes.data),
                                        ctypes.c_size_t(buf.size)) == INVALID  # null tensors


@pytest.mark.parametrize("K0", [882, 49])
@pytest.mark.parametrize("wdtype", [F32, F16])
def test_blob_holds_every_weight(lib, K0, wdtype):
    P = update_ref.formula_params(K0)
    st, blob = pack(lib, P, K0, wdtype)
    assert st == OK
    hdr = blob[:16].view(np.int32)
    Kpad = (K0 + 127) // 128 * 128
    assert bytes(blob[:4]) == b"UPD1" and list(hdr[1:4]) == [wdtype, K0, Kpad]
    es = 2 if wdtype == F16 else 4
    wt = np.float16 if wdtype == F16 else np.float32
    off = HDR
    for li, name in enumerate(LAYERS):
        K, Kp = (K0, Kpad) if li == 0 else (DIM, DIM)
        W = unpack_layer(blob, off, K, Kp, wdtype)
        want = P[name + ".weight"].astype(wt)  # numpy rounds to nearest even
        assert np.array_equal(W[:, :K], want), name
        assert not W[:, K:].any(), name + ": padded K tail must be zero"
        off += DIM * Kp * es
    V = blob[off:off + (19 + 8 + 4) * DIM * 4 + 16].view(np.float32)
    for li, name in enumerate(LAYERS):
        assert np.array_equal(V[li * DIM:(li + 1) * DIM], P[name + ".bias"]), name
    o = 19 * DIM
    for name in NORMS:
        assert np.array_equal(V[o:o + DIM], P[name + ".weight"]), name
        assert np.array_equal(V[o + DIM:o + 2 * DIM], P[name + ".bias"]), name
        o += 2 * DIM
    for name in ("d.1", "w.1"):
        want = P[name + ".weight"].astype(wt).astype(np.float32).reshape(-1)
        assert np.array_equal(V[o:o + 2 * DIM], want), name
        o += 2 * DIM
    assert np.array_equal(V[o:o + 2], P["d.1.bias"]) and np.array_equal(V[o + 2:o + 4], P["w.1.bias"])
    assert off + (o + 4) * 4 <= blob.size == lib.dpvo_update_packed_bytes(K0, wdtype)
