"""CPU: dpvo_kf_motion, dpvo_kf_shift and dpvo_edges_loop validate their
arguments before any launch -- no GPU needed.  Every call here is refused on
the host; none reaches a kernel."""
import ctypes

import pytest

INVALID, UNSUPPORTED = 1, 3
ONE = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    vp, i, d, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
    lib.dpvo_kf_motion.argtypes = [vp] * 7 + [i, vp, i, d, vp, vp, vp]
    lib.dpvo_kf_shift.argtypes = [vp, i, vp, vp, vp, vp, vp, i, vp, vp, vp, i] + [vp] * 5 + [i, vp]
    lib.dpvo_edges_loop.argtypes = ([vp] * 4 + [i, i, vp, i, vp, i, i, i, i, f, i, i] + [vp] * 5 +
                                    [vp])
    return lib


def _motion(lib, ptrs=None, P=3, ki=18, thresh=12.5):
    p = [ONE] * 10 if ptrs is None else ptrs
    return lib.dpvo_kf_motion(p[0], p[1], p[2], p[3], p[4], p[5], p[6], P, p[7], ki, thresh, p[8],
                              p[9], None)


def test_kf_motion_validation(lib):
    # keyframe_index - 1 frames move in a drop; the shift holds 16
    for ki in (18, 19, 100, 1 << 30):
        assert _motion(lib, ki=ki) == UNSUPPORTED, ki
    for k in range(10):
        ptrs = [ONE] * 10
        ptrs[k] = None
        assert _motion(lib, ptrs) == INVALID, k
    assert _motion(lib, P=0) == INVALID and _motion(lib, P=-1) == INVALID
    assert _motion(lib, ki=0) == INVALID and _motion(lib, ki=-3) == INVALID


def _shift(lib, ptrs=None, M=4, max_edges=64, arrays=None, narrays=None, delta=(None,) * 5,
           delta_cap=4):
    """arrays: list of (pointer, bytes per frame, ring) read on the host"""
    p = [ONE] * 6 if ptrs is None else ptrs
    arrays = [] if arrays is None else arrays
    n = len(arrays) if narrays is None else narrays
    fa = (ctypes.c_void_p * max(len(arrays), 1))(*[a[0] for a in arrays])
    by = (ctypes.c_int64 * max(len(arrays), 1))(*[a[1] for a in arrays])
    rg = (ctypes.c_int32 * max(len(arrays), 1))(*[a[2] for a in arrays])
    have = bool(arrays)
    return lib.dpvo_kf_shift(p[0], M, p[1], p[2], p[3], p[4], p[5], max_edges,
                             fa if have else None, by if have else None, rg if have else None, n,
                             *delta, delta_cap, None)


def test_kf_shift_validation(lib):
    ok = (16, 28, 0)
    for k in range(6):  # kf, st, ii, jj, kk, counts
        ptrs = [ONE] * 6
        ptrs[k] = None
        assert _shift(lib, ptrs, arrays=[(None, 4, 0)]) == INVALID, k
    assert _shift(lib, M=0, arrays=[(None, 4, 0)]) == INVALID
    assert _shift(lib, max_edges=0, arrays=[(None, 4, 0)]) == INVALID
    assert _shift(lib, narrays=-1) == INVALID
    assert _shift(lib, narrays=2) == INVALID  # arrays announced, tables missing
    # kMaxShift = 12 arrays travel in the launch argument
    assert _shift(lib, arrays=[ok] * 13) == UNSUPPORTED
    assert _shift(lib, arrays=[ok] * 40) == UNSUPPORTED
    # per-array checks, at 12 and below (the refusal comes before the launches)
    for bad in ((None, 28, 0), (16, 0, 0), (16, -4, 0), (16, 28, -1)):
        assert _shift(lib, arrays=[ok] * 11 + [bad]) == INVALID, bad
        assert _shift(lib, arrays=[bad]) == INVALID, bad
    # the delta log: all of log, tstamps, count, poses, tstamps of the frames, or none (each
    # call also carries a refused array, so that none can reach a launch)
    full = [ONE] * 5  # poses, tstamps, delta_log, delta_tstamps, delta_count
    for k in range(5):
        d = list(full)
        d[k] = None
        assert _shift(lib, arrays=[(None, 4, 0)], delta=tuple(d)) == INVALID, k
    assert _shift(lib, arrays=[(None, 4, 0)], delta=tuple(full), delta_cap=0) == INVALID


def _loop(lib, ptrs=None, P=3, M=4, n_cap=128, rw=20, age=1000, gof=15, ki=-1, thresh=64.0,
          max_edges=1000, nms=1):
    """keyframe_index defaults to a refused value: no call of this file may
    reach a launch"""
    p = [ONE] * 11 if ptrs is None else ptrs
    return lib.dpvo_edges_loop(p[0], p[1], p[2], p[3], P, M, p[4], n_cap, p[5], rw, age, gof, ki,
                               thresh, max_edges, nms, p[6], p[7], p[8], p[9], p[10], None)


def test_edges_loop_validation(lib):
    # poses, patches, intrinsics, ix, st, [last_global_ba], work, kk, jj, count, [errors]
    for k in (0, 1, 2, 3, 4, 6, 7, 8, 9):
        ptrs = [ONE] * 11
        ptrs[k] = None
        assert _loop(lib, ptrs, ki=4, max_edges=1025) == INVALID, k
    for k in (5, 10):  # optional: validation goes on to the caps
        ptrs = [ONE] * 11
        ptrs[k] = None
        assert _loop(lib, ptrs, ki=4, max_edges=1025) == UNSUPPORTED, k
    # every call below also exceeds a cap: INVALID comes first, and nothing can reach a launch
    for bad in (dict(P=1), dict(P=0), dict(M=0), dict(n_cap=-1), dict(rw=-1), dict(age=-1),
                dict(nms=-1), dict(max_edges=-1)):
        kw = dict(n_cap=1 << 30) if "max_edges" in bad else dict(max_edges=1025)
        assert _loop(lib, ki=4, **kw, **bad) == INVALID, bad
    # target frames [n - global_opt_freq, n - keyframe_index) for n > removal_window
    assert _loop(lib, ki=-1, max_edges=1025) == INVALID
    assert _loop(lib, ki=-1, gof=-5, max_edges=1025) == INVALID
    assert _loop(lib, ki=4, rw=20, gof=22, max_edges=1025) == INVALID
    assert _loop(lib, ki=4, rw=0, gof=2, max_edges=1025) == INVALID
    assert _loop(lib, ki=4, rw=5, gof=8, max_edges=1025) == INVALID
    # global_opt_freq == removal_window + 1 and keyframe_index == 0 pass on to the caps
    assert _loop(lib, ki=0, rw=20, gof=21, max_edges=1025) == UNSUPPORTED


def test_edges_loop_caps(lib):
    # sort size: (gof - ki) x min(n_cap - rw, age) <= 16384
    assert _loop(lib, ki=4, gof=15, n_cap=2000, age=1500) == UNSUPPORTED  # 11 x 1500
    assert _loop(lib, ki=4, gof=20, rw=20, n_cap=1045, age=1025) == UNSUPPORTED  # 16 x 1025
    assert _loop(lib, ki=4, gof=20, rw=20, n_cap=2000, age=1025) == UNSUPPORTED
    # suppression bitmap: n_cap x (gof - ki) <= 131072 bits
    assert _loop(lib, ki=4, gof=15, n_cap=11916, age=1) == UNSUPPORTED  # 131076
    assert _loop(lib, ki=4, gof=15, n_cap=1 << 30, age=1) == UNSUPPORTED
    # accepted-edge list
    assert _loop(lib, ki=4, max_edges=1025) == UNSUPPORTED
    assert _loop(lib, ki=4, max_edges=1 << 30) == UNSUPPORTED
