"""CPU: the C ABI of the update operator's training surface (include/dpvo_hot.h:
dpvo_update_saved_bytes, dpvo_update_forward_train,
dpvo_update_backward_workspace_bytes, dpvo_update_backward,
dpvo_update_pack_weights_device, dpvo_update_saved_relu_masks): size functions
and the status rules, all of which are decided before any launch, so they run
without a device."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, F16, F64 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    for f in ("dpvo_update_saved_bytes", "dpvo_update_backward_workspace_bytes",
              "dpvo_update_workspace_bytes", "dpvo_update_packed_bytes"):
        getattr(lib, f).restype = ctypes.c_size_t
    return lib


one = ctypes.c_void_p(64)
big = ctypes.c_size_t(1 << 40)
sz = ctypes.c_size_t


def ptrs50(null_at=None):
    a = (ctypes.c_void_p * 50)(*[64] * 50)
    if null_at is not None:
        a[null_at] = None
    return a


def test_sizes(lib):
    sb, bw = lib.dpvo_update_saved_bytes, lib.dpvo_update_backward_workspace_bytes
    for E, K0 in [(0, 882), (-1, 882), (200, 0), (200, -5)]:
        assert sb(E, K0) == 0 and bw(E, K0) == 0, (E, K0)
    seq = [(1, 49), (17, 49), (17, 882), (200, 882), (4097, 882), (9850, 882)]
    for f in (sb, bw):
        v = [f(E, K0) for E, K0 in seq]
        assert all(0 < a < b for a, b in zip(v, v[1:])), v
    # 25 planes of [E, 384] fp32, corr, w and twelve int arrays of the two plans
    for E, K0 in seq:
        assert sb(E, K0) >= E * (25 * 384 * 4 + 4 * K0 + 8 + 48)
        assert sb(E, K0) <= E * (25 * 384 * 4 + 4 * K0 + 8 + 48) + 40 * 256 + 96
        assert bw(E, K0) >= 6 * E * 384 * 4 + ((E + 511) // 512) * 384 * max(K0, 384) * 4


def test_forward_train_status_rules_without_a_device(lib):
    f = lib.dpvo_update_forward_train
    names = ("blob", "net", "inp", "corr", "ix", "jx", "ws", "saved", "net_out", "d", "w")

    def call(wd=F32, E=200, dim=384, K0=882, io=F32, wbytes=big, sbytes=big, **null):
        p = {k: one for k in names}
        p.update({k: None for k in null})
        return f(p["blob"], wd, p["net"], p["inp"], p["corr"], p["ix"], p["jx"], E, dim, K0, io,
                 p["ws"], wbytes, p["saved"], sbytes, p["net_out"], p["d"], p["w"], None)

    for name in names:
        assert call(**{name: 1}) == INVALID, name
    assert call(dim=128) == UNSUPPORTED and call(wd=F16) == UNSUPPORTED
    assert call(io=F16) == UNSUPPORTED and call(wd=F16, io=F16) == UNSUPPORTED
    assert call(io=F64) == UNSUPPORTED
    assert call(K0=0) == INVALID and call(K0=-3) == INVALID
    assert call(E=0) == OK and call(E=-2) == OK
    assert call(E=0, net=1, wbytes=sz(0), sbytes=sz(0)) == OK  # no launch, nothing read
    for E, K0 in [(17, 49), (200, 882)]:
        ws, sv = lib.dpvo_update_workspace_bytes(E, K0), lib.dpvo_update_saved_bytes(E, K0)
        assert call(E=E, K0=K0, wbytes=sz(ws - 1)) == WORKSPACE
        assert call(E=E, K0=K0, sbytes=sz(sv - 1)) == WORKSPACE
        assert call(E=E, K0=K0, wbytes=sz(0), sbytes=sz(0)) == WORKSPACE
    # the order: unsupported, K0, E <= 0, null pointers, sizes
    assert call(dim=128, K0=0, saved=1, sbytes=sz(0)) == UNSUPPORTED
    assert call(K0=0, saved=1, sbytes=sz(0)) == INVALID
    assert call(saved=1, sbytes=sz(0)) == INVALID


def test_backward_status_rules_without_a_device(lib):
    f = lib.dpvo_update_backward
    req = ("saved", "ix", "jx", "ws")
    opt = ("g_net_out", "g_d", "g_w", "g_net", "g_inp", "g_corr")

    def call(dim=384, K0=882, E=200, sbytes=big, wbytes=big, parr="ok", garr="ok", **null):
        p = {k: one for k in req + opt}
        p.update({k: None for k in null})
        pa = ptrs50() if parr == "ok" else parr
        ga = ptrs50() if garr == "ok" else garr
        return f(pa, dim, K0, p["saved"], sbytes, p["ix"], p["jx"], E, p["g_net_out"], p["g_d"],
                 p["g_w"], p["g_net"], p["g_inp"], p["g_corr"], ga, p["ws"], wbytes, None)

    for name in req:
        assert call(**{name: 1}) == INVALID, name
    assert call(parr=None) == INVALID
    for k in (0, 13, 49):
        assert call(parr=ptrs50(k)) == INVALID
        assert call(garr=ptrs50(k)) == INVALID
    assert call(dim=256) == UNSUPPORTED and call(dim=0) == UNSUPPORTED
    assert call(K0=0) == INVALID
    assert call(E=0) == OK and call(E=-1) == OK and call(E=0, saved=1, wbytes=sz(0)) == OK
    for E, K0 in [(17, 49), (200, 882)]:
        sv, ws = lib.dpvo_update_saved_bytes(E, K0), lib.dpvo_update_backward_workspace_bytes(E, K0)
        assert call(E=E, K0=K0, sbytes=sz(sv - 1)) == WORKSPACE
        assert call(E=E, K0=K0, wbytes=sz(ws - 1)) == WORKSPACE
        # optional cotangents, outputs and parameter gradients: still decided by the sizes
        assert call(E=E, K0=K0, wbytes=sz(ws - 1), garr=None,
                    **{k: 1 for k in opt}) == WORKSPACE
    assert call(dim=256, K0=0, saved=1) == UNSUPPORTED
    assert call(K0=0, saved=1, sbytes=sz(0)) == INVALID
    assert call(saved=1, sbytes=sz(0)) == INVALID


def test_pack_weights_device_status_rules_without_a_device(lib):
    f = lib.dpvo_update_pack_weights_device

    def call(params="ok", dim=384, K0=882, wd=F32, blob=one, nbytes=big):
        return f(ptrs50() if params == "ok" else params, dim, K0, wd, blob, nbytes, None)

    assert call(params=None) == INVALID and call(blob=None) == INVALID
    for k in (0, 25, 49):
        assert call(params=ptrs50(k)) == INVALID
    assert call(dim=128) == UNSUPPORTED and call(wd=2) == UNSUPPORTED and call(wd=-1) == UNSUPPORTED
    assert call(K0=0) == INVALID
    for wd in (F32, F16):
        for K0 in (49, 882):
            need = lib.dpvo_update_packed_bytes(K0, wd)
            assert call(K0=K0, wd=wd, nbytes=sz(need - 1)) == WORKSPACE
    assert call(dim=128, blob=None, nbytes=sz(0)) == UNSUPPORTED
    assert call(blob=None, nbytes=sz(0)) == INVALID


def test_relu_masks_status_rules_without_a_device(lib):
    f = lib.dpvo_update_saved_relu_masks

    def call(saved=one, sbytes=big, E=200, K0=882, masks=one):
        return f(saved, sbytes, E, K0, masks, None)

    assert call(saved=None) == INVALID and call(masks=None) == INVALID
    assert call(K0=0) == INVALID
    assert call(E=0) == OK and call(E=0, saved=None) == OK
    need = lib.dpvo_update_saved_bytes(200, 882)
    assert call(sbytes=sz(need - 1)) == WORKSPACE and call(saved=None, sbytes=sz(0)) == INVALID
