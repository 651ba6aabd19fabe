"""CPU: return code and precedence of every rejection of the training C ABI
(dpvo_transform_*, dpvo_flow_loss_*, dpvo_pose_loss_*), with dummy pointers.
The order is: unsupported shape (3), nothing to do (0), null pointer (1),
workspace size (4).  Every call returns on the host, before any launch."""
import ctypes

import pytest

one = ctypes.c_void_p(1)
big = ctypes.c_size_t(1 << 40)


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    L = dpvo_amd.c_abi()
    L.dpvo_transform_workspace_bytes.restype = ctypes.c_size_t
    return L


def tf_fwd(lib, E=10, P=3, N=4, M=6, ptr=one):
    return lib.dpvo_transform_forward(ptr, ptr, ptr, ptr, ptr, ptr, E, P, N, M, ptr, ptr, None, None)


def tf_bwd(lib, E=10, P=3, N=4, M=6, ptr=one, ws=big, gp=one, gk=one):
    return lib.dpvo_transform_backward(ptr, ptr, ptr, ptr, ptr, ptr, E, P, N, M, ptr, gp, gk, ptr,
                                       ws, None)


def fl_fwd(lib, E=10, P=3, ptr=one):
    return lib.dpvo_flow_loss_forward(ptr, ptr, ptr, E, P, ptr, ptr, ptr, ptr, None)


def fl_bwd(lib, E=10, P=3, ptr=one):
    return lib.dpvo_flow_loss_backward(ptr, ptr, ptr, ptr, ptr, ptr, E, P, ptr, None)


def pl_fwd(lib, n=5, ptr=one):
    return lib.dpvo_pose_loss_forward(ptr, ptr, n, ptr, ptr, ptr, None)


def pl_bwd(lib, n=5, ptr=one):
    return lib.dpvo_pose_loss_backward(ptr, ptr, n, ptr, ptr, None)


@pytest.mark.parametrize("call", [tf_fwd, tf_bwd, fl_fwd, fl_bwd])
def test_edge_entries(lib, call):
    # UNSUPPORTED: P other than 1 or 3, before everything else
    for P in (2, 0, 5, -3):
        assert call(lib, P=P) == 3
        assert call(lib, P=P, E=0, ptr=None) == 3
    # nothing to do: OK whatever the pointers are
    assert call(lib, E=0, ptr=None) == 0
    assert call(lib, E=-1, ptr=None) == 0
    assert call(lib, E=0, P=1, ptr=None) == 0
    # INVALID: null pointers
    assert call(lib, ptr=None) == 1
    assert call(lib, P=1, ptr=None) == 1
    # the index range: E P P must stay below 2^30
    assert call(lib, E=(1 << 30) // 9 + 1, ptr=None) == 3
    assert call(lib, E=(1 << 30) // 9, ptr=None) == 1


def test_transform_backward_workspace_and_order(lib):
    w = lib.dpvo_transform_workspace_bytes
    need = w(10, 3)
    assert need == 10 * (12 + 27) * 8
    # (that exactly `need` bytes are accepted is checked with real buffers in
    # test_transform_gpu.py: no call here may pass every check with these pointers)
    assert tf_bwd(lib, ws=ctypes.c_size_t(need - 1), ptr=None) == 1  # null before workspace
    # one byte short with valid-looking pointers is rejected on the host: the
    # only non-null arguments that would be touched are never reached
    assert lib.dpvo_transform_backward(one, one, one, one, one, one, 10, 3, 4, 6, one, one, one,
                                       one, ctypes.c_size_t(need - 1), None) == 4
    assert lib.dpvo_transform_backward(one, one, one, one, one, one, 10, 2, 4, 6, one, one, one,
                                       one, ctypes.c_size_t(0), None) == 3  # unsupported first
    # no gradient wanted: nothing to do, before the null and the size checks
    assert tf_bwd(lib, gp=None, gk=None, ptr=None, ws=ctypes.c_size_t(0)) == 0
    # N, M < 1 with an edge to process: INVALID
    assert lib.dpvo_transform_backward(one, one, one, one, one, one, 10, 3, 0, 6, one, one, one,
                                       one, big, None) == 1
    assert lib.dpvo_transform_forward(one, one, one, one, one, one, 10, 3, 4, 0, one, one, None,
                                      None) == 1


def test_transform_workspace_bytes(lib):
    w = lib.dpvo_transform_workspace_bytes
    assert w(0, 3) == 0 and w(-5, 3) == 0 and w(0, 1) == 0
    assert w(10, 2) == 0
    for P in (1, 3):
        sizes = [w(E, P) for E in (1, 2, 63, 64, 65, 257, 4320, 18000)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert w(100, 1) < w(100, 3)


@pytest.mark.parametrize("call", [pl_fwd, pl_bwd])
def test_pose_entries(lib, call):
    assert call(lib, n=33) == 3
    assert call(lib, n=33, ptr=None) == 3  # unsupported before null
    assert call(lib, n=1000) == 3
    assert call(lib, n=1, ptr=None) == 0   # nothing to do before null
    assert call(lib, n=0, ptr=None) == 0
    assert call(lib, n=-2, ptr=None) == 0
    assert call(lib, n=2, ptr=None) == 1
    assert call(lib, n=32, ptr=None) == 1
