"""CPU: return code and precedence of every rejection of dpvo_spd_solve, with
dummy pointers: INVALID (1) for negative sizes, OK for an empty problem, then
INVALID for null or contradictory pointers, then UNSUPPORTED (3) for the dtype
and for a size whose column scratch does not fit the default LDS.  Every call
here is rejected or returns on the host; no accepted size appears."""
import ctypes

import pytest

F32, F16, F64 = 0, 1, 2
OK, INVALID, UNSUPPORTED = 0, 1, 3
one = ctypes.c_void_p(1)
# the first n past the HBM path's limit: lv[n] alone beyond 64 KB - 64 B
PAST = {F64: 8184 + 1, F32: 16368 + 1}


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    return dpvo_amd.c_abi()


def solve(lib, H=one, B=one, L=one, X=one, info=one, batch=2, n=8, k=1, factor=1, dtype=F64):
    return lib.dpvo_spd_solve(H, B, L, X, info, batch, n, k, factor, dtype, None)


def test_sizes(lib):
    assert solve(lib, batch=-1) == INVALID
    assert solve(lib, n=-1) == INVALID
    assert solve(lib, k=-1) == INVALID
    # negative sizes win over the empty problem, the empty problem over everything else
    assert solve(lib, batch=0, n=-1) == INVALID
    assert solve(lib, batch=-1, n=0) == INVALID
    assert solve(lib, H=None, B=None, L=None, X=None, info=None, batch=0) == OK
    assert solve(lib, H=None, B=None, L=None, X=None, info=None, n=0) == OK
    assert solve(lib, H=None, B=None, L=None, X=None, info=None, n=0, dtype=F16) == OK
    assert solve(lib, batch=0, factor=0) == OK  # ... the solve-only rule about L included


def test_pointers(lib):
    assert solve(lib, H=None) == INVALID
    assert solve(lib, X=None) == INVALID
    assert solve(lib, B=None) == INVALID
    assert solve(lib, B=None, k=3) == INVALID
    # solve-only reads H as the factor: a factor buffer contradicts it
    assert solve(lib, factor=0, L=one, info=None) == INVALID
    assert solve(lib, factor=0, L=one, info=None, dtype=F32) == INVALID


def test_dtype(lib):
    assert solve(lib, dtype=F16) == UNSUPPORTED
    assert solve(lib, dtype=7) == UNSUPPORTED
    assert solve(lib, dtype=-1) == UNSUPPORTED
    assert solve(lib, dtype=F16, factor=0, L=None, info=None) == UNSUPPORTED
    # null pointers win over the dtype, and so does the solve-only rule
    assert solve(lib, dtype=F16, H=None) == INVALID
    assert solve(lib, dtype=7, X=None) == INVALID
    assert solve(lib, dtype=F16, B=None) == INVALID
    assert solve(lib, dtype=F16, factor=0, L=one) == INVALID


@pytest.mark.parametrize("dtype,n", [(F64, 143), (F32, 202)])
def test_factor_beyond_lds_needs_the_factor_buffer(lib, dtype, n):
    """The first size of each dtype whose working copy is the caller's L."""
    assert solve(lib, dtype=dtype, n=n, L=None) == INVALID
    assert solve(lib, dtype=dtype, n=n, L=None, batch=1, info=None) == INVALID


@pytest.mark.parametrize("dtype", [F64, F32])
def test_first_size_past_the_limit(lib, dtype):
    n = PAST[dtype]
    assert solve(lib, dtype=dtype, n=n, batch=1) == UNSUPPORTED
    assert solve(lib, dtype=dtype, n=n, batch=1, factor=0, L=None, info=None) == UNSUPPORTED
    assert solve(lib, dtype=dtype, n=n, batch=3, k=2) == UNSUPPORTED
    assert solve(lib, dtype=dtype, n=1 << 20, batch=1) == UNSUPPORTED
    # INVALID still first: no factor buffer, null input
    assert solve(lib, dtype=dtype, n=n, batch=1, L=None) == INVALID
    assert solve(lib, dtype=dtype, n=n, batch=1, H=None) == INVALID


def test_the_layer_admits_what_the_solve_can_launch():
    """6 n_free of the BA layer's boundary (test_ba_layer_capi.py: 1364 free
    poses accepted, 1365 rejected) against the fp64 limit."""
    assert 6 * 1364 == PAST[F64] - 1 and 6 * 1365 > PAST[F64] - 1
