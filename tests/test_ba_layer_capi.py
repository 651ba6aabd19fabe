"""CPU: return code and precedence of every rejection of the BA-layer C ABI
(dpvo_ba_layer_*), with dummy pointers: OK for E <= 0 first, then INVALID (1),
then UNSUPPORTED (3), then WORKSPACE (4).  Every call is rejected on the host."""
import ctypes

import pytest

F32, F16, F64 = 0, 1, 2
one = ctypes.c_void_p(1)
big, small = ctypes.c_size_t(1 << 40), ctypes.c_size_t(16)
bounds = (ctypes.c_double * 4)(0.0, 0.0, 159.0, 119.0)


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    L = dpvo_amd.c_abi()
    L.dpvo_ba_layer_workspace_bytes.restype = ctypes.c_size_t
    return L


def fwd(lib, E=10, M=20, p=3, N=8, n=5, fixedp=1, so=0, dtype=F64, ws=big, ptr=one):
    return lib.dpvo_ba_layer_forward(ptr, ptr, ptr, ptr, ptr, None, ctypes.c_double(1e-4), ptr, ptr,
                                     ptr, E, M, p, N, n, fixedp, so, bounds, ctypes.c_double(100.0),
                                     dtype, ptr, ptr, ptr, ws, 1, None)


def bwd(lib, E=10, M=20, p=3, N=8, n=5, fixedp=1, so=0, dtype=F64, ws=big, ptr=one):
    return lib.dpvo_ba_layer_backward(ptr, ptr, ptr, ptr, ptr, E, M, p, N, n, fixedp, so, dtype, ptr,
                                      ptr, ptr, ptr, ptr, ws, None)


@pytest.mark.parametrize("call", [fwd, bwd])
def test_rejections_and_precedence(lib, call):
    # E <= 0 is an OK no-op whatever else is wrong
    assert call(lib, E=0, n=0, fixedp=3, p=2, dtype=F16, ws=small, ptr=None) == 0
    assert call(lib, E=-1) == 0
    # INVALID: n < fixedp, p even or < 1, dtype not F32 / F64, n > N, null pointers
    assert call(lib, n=1, fixedp=2) == 1
    assert call(lib, p=2) == 1
    assert call(lib, p=0) == 1
    assert call(lib, p=-3) == 1
    assert call(lib, dtype=F16) == 1
    assert call(lib, dtype=7) == 1
    assert call(lib, n=9) == 1
    assert call(lib, ptr=None) == 1
    # UNSUPPORTED: 6 n_free beyond dpvo_spd_solve's limit, 8184 (1365 free poses)
    assert call(lib, N=2000, n=1366, fixedp=1) == 3
    assert call(lib, N=2000, n=1365, fixedp=1, ws=small) == 4   # 6 * 1364 = 8184 is accepted
    assert call(lib, N=2000, n=1366, fixedp=1, so=1, ws=small) == 4  # structure only: no pose system
    # WORKSPACE
    assert call(lib, ws=small) == 4
    # precedence: INVALID wins over UNSUPPORTED and WORKSPACE, UNSUPPORTED over WORKSPACE
    assert call(lib, N=2000, n=1366, p=2, ws=small) == 1
    assert call(lib, N=2000, n=1366, dtype=F16, ws=small) == 1
    assert call(lib, n=1, fixedp=2, ws=small) == 1
    assert call(lib, N=2000, n=1366, ws=small) == 3


def test_workspace_bytes(lib):
    w = lib.dpvo_ba_layer_workspace_bytes
    assert w(-1, 1, 1, 0) == 0
    f, b = w(1000, 300, 10, 0), w(1000, 300, 10, 1)
    assert 0 < f < b
    # the dense part is sized by the free poses, never by the pose buffer
    assert w(1000, 300, 10, 1) == b and w(1000, 300, 11, 1) > b
    # one byte short of the advertised size is rejected
    assert fwd(lib, E=1000, M=300, n=11, N=11, fixedp=1, ws=ctypes.c_size_t(b - 1)) == 4
