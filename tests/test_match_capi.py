"""CPU: dpvo_match_descriptors and dpvo_triangulate_tracks validate their
arguments before any launch -- no GPU needed -- and the public names exist."""
import ctypes

import pytest

INVALID, UNSUPPORTED, WORKSPACE = 1, 3, 4
ONE = ctypes.c_void_p(16)  # a non-null, 16-byte aligned pointer that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    lib.dpvo_match_workspace_bytes.argtypes = [i, i]
    lib.dpvo_match_workspace_bytes.restype = sz
    lib.dpvo_match_descriptors.argtypes = ([vp, vp] + [i] * 5 + [vp, i, vp, f, f] + [vp] * 6 +
                                           [sz, vp])
    lib.dpvo_triangulate_tracks.argtypes = ([vp, vp, vp, i, i, vp, i, vp, i, vp, i, vp, vp, f, f,
                                             i, f] + [vp] * 6)
    return lib


def test_exports_exist(lib):
    for name in ("dpvo_match_descriptors", "dpvo_match_workspace_bytes", "dpvo_triangulate_tracks"):
        assert hasattr(lib, name), name


def _match(lib, ptrs=None, dtype=0, N0=8, N1=9, D=32, n0=8, n0_dev=None, n1=9, n1_dev=None,
           r2=0.64, md2=1.0, ws=1 << 20):
    p = [ONE] * 8 if ptrs is None else ptrs
    return lib.dpvo_match_descriptors(p[0], p[1], dtype, N0, N1, D, n0, n0_dev, n1, n1_dev, r2,
                                      md2, p[2], p[3], p[4], p[5], p[6], p[7], ws, None)


def test_match_validation(lib):
    for k in range(8):
        ptrs = [ONE] * 8
        ptrs[k] = None
        assert _match(lib, ptrs) == INVALID, k
    for D in (0, 2, 6, 33, 130, -4):
        assert _match(lib, D=D) == INVALID, D
    assert _match(lib, N0=0, n0=0) == INVALID
    assert _match(lib, N1=-1, n1=0) == INVALID
    assert _match(lib, dtype=2) == INVALID  # fp64 descriptors
    assert _match(lib, n0=9) == INVALID and _match(lib, n0=-1) == INVALID
    assert _match(lib, n1=10) == INVALID
    assert _match(lib, r2=-0.5) == INVALID and _match(lib, r2=float("nan")) == INVALID
    assert _match(lib, md2=-1.0) == INVALID
    ptrs = [ONE] * 8
    ptrs[0] = ctypes.c_void_p(20)  # rows not aligned to four fp32 elements
    assert _match(lib, ptrs) == INVALID
    assert _match(lib, ptrs, dtype=1) == INVALID  # nor to four fp16 elements
    ptrs[0] = ctypes.c_void_p(24)
    assert _match(lib, ptrs) == INVALID and _match(lib, ptrs, dtype=1, ws=0) == WORKSPACE
    assert _match(lib, N0=4097, n0=8) == UNSUPPORTED
    assert _match(lib, N1=4097) == UNSUPPORTED
    assert _match(lib, D=260) == UNSUPPORTED
    # a device limit replaces the host one, which is then not looked at
    assert _match(lib, n0=99, n0_dev=ONE, ws=0) == WORKSPACE
    need = lib.dpvo_match_workspace_bytes(8, 9)
    assert need == 6 * 64 * 4  # one 64 x 64 tile: three planes of row and of column triples
    assert lib.dpvo_match_workspace_bytes(2048, 2048) == 6 * 32 * 32 * 64 * 4
    assert lib.dpvo_match_workspace_bytes(0, 5) == 0 and lib.dpvo_match_workspace_bytes(5, 4097) == 0
    assert _match(lib, ws=need - 1) == WORKSPACE


def _tri(lib, ptrs=None, stride=9, M=8, N0=5, N1=6, N2=7, max_depth=20.0, max_residual=2.0,
         iterations=6, lmbda=1e-3):
    p = [ONE] * 13 if ptrs is None else ptrs
    return lib.dpvo_triangulate_tracks(p[0], p[1], p[2], stride, M, p[3], N0, p[4], N1, p[5], N2,
                                       p[6], p[7], max_depth, max_residual, iterations, lmbda,
                                       p[8], p[9], p[10], p[11], p[12], None)


def test_triangulate_validation(lib):
    for k in range(13):
        ptrs = [ONE] * 13
        ptrs[k] = None
        assert _tri(lib, ptrs) == INVALID, k
    for name in ("stride", "M", "N0", "N1", "N2"):
        assert _tri(lib, **{name: 0}) == INVALID, name
        assert _tri(lib, **{name: -2}) == INVALID, name
    assert _tri(lib, iterations=-1) == INVALID
    assert _tri(lib, lmbda=-1.0) == INVALID and _tri(lib, lmbda=float("nan")) == INVALID
    assert _tri(lib, M=1025) == UNSUPPORTED
    assert _tri(lib, N1=4097) == UNSUPPORTED
