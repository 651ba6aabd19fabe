"""CPU: the native build loads and exposes the full boundary (no GPU compute)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dpvo_hot.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dpvo_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    return dpvo_amd.c_abi()


def test_header_declares_entry_points():
    names = declared_functions()
    for must in ["dpvo_corr_forward", "dpvo_corr_backward", "dpvo_patchify_forward",
                 "dpvo_patchify_backward", "dpvo_ba_forward", "dpvo_reproject", "dpvo_neighbors",
                 "dpvo_lie_forward", "dpvo_lie_backward", "dpvo_corr_forward_levels",
                 "dpvo_ba_build_schur", "dpvo_ba_solve_update"]:
        assert must in names


def test_library_exports_every_declared_symbol(lib):
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing


def test_status_and_version(lib):
    assert lib.dpvo_version().startswith(b"dpvo_hot gfx950")
    assert lib.dpvo_status_string(0) == b"ok"
    assert lib.dpvo_status_string(3) == b"unsupported configuration"


def test_host_side_argument_validation(lib):
    # invalid arguments are rejected before any kernel launch (no GPU needed)
    f = lib.dpvo_corr_forward
    # radius 8 > 7 -> DPVO_ERR_INVALID
    assert f(None, None, None, None, None, 1, 4, 128, 3, 3, 1, 1, 10, 10, 8, 0, None, None) == 1
    # patch of 5x5 = 25 pixels > 16 -> DPVO_ERR_UNSUPPORTED
    assert f(None, None, None, None, None, 1, 4, 128, 5, 5, 1, 1, 10, 10, 3, 0, None, None) == 3
    # zero edges is a no-op success
    assert f(None, None, None, None, None, 1, 0, 128, 3, 3, 1, 1, 10, 10, 3, 0, None, None) == 0
    # BA: t1 < t0 invalid; too many free poses unsupported; workspace too small
    ba_setup = lib.dpvo_ba_setup
    one = ctypes.c_void_p(1)
    assert ba_setup(one, one, one, 10, 100, 5, 4, one, ctypes.c_size_t(1 << 30), None) == 1
    assert ba_setup(one, one, one, 10, 100, 0, 64, one, ctypes.c_size_t(1 << 30), None) == 3
    assert ba_setup(one, one, one, 10, 100, 0, 4, one, ctypes.c_size_t(16), None) == 4
    assert lib.dpvo_lie_forward(2, 0, 0, 4, None, None, None, None) == 3  # RxSO3 not built


def test_ba_and_reproject_return_codes(lib):
    """Return code of every dpvo_ba_* / dpvo_reproject_* export, and which
    check wins where two apply: OK for E <= 0 first, then INVALID (1), then
    UNSUPPORTED (3), then WORKSPACE (4).  Every call is rejected on the host:
    the pointers are dummies, and calls that the window path would accept on a
    device get a 16-byte workspace.  The literals were recorded from the build
    before the dispatch was refactored.  (dpvo_ba_set_status_sink is left out:
    it re-points the process-wide status sink.)"""
    one, big, small = ctypes.c_void_p(1), ctypes.c_size_t(1 << 30), ctypes.c_size_t(16)
    # without a device the window path supports nothing; with one it supports
    # E = 256, N = 7, and then the short workspace is what rejects the call
    window = lib.dpvo_ba_plan_supported(256, 1, 8, 3)
    assert window in (0, 1)
    declined = 4 if window else 3
    edges, ba = (one,) * 6, (one,) * 9  # poses .. kk without / with target, weight, lmbda
    out5 = (ctypes.c_int64 * 5)()

    wsb = lib.dpvo_ba_workspace_bytes
    if window:
        # the sizes depend on the device: the window scratch lies behind the
        # multi-kernel layout, and the large-graph layout holds the sort's scratch
        assert wsb(256, 1, 8) > 139776
        assert lib.dpvo_ba_plan_offsets(256, 1, 8, out5) == 0 and out5[0] == 139776
        assert wsb(20000, 0, 8) > 0 and wsb(256, 0, 30) > 0
    else:
        assert wsb(256, 1, 8) == 139776
        assert lib.dpvo_ba_plan_offsets(256, 1, 8, out5) == 3
        assert wsb(20000, 0, 8) == 135297536  # E > 16384: large-graph layout
        assert wsb(256, 0, 30) == 109400576   # N > 20: large-graph layout
    assert [lib.dpvo_ba_select_path(m) for m in (-1, 1, 3, 6, 0)] == [1, 1, 1, 1, 0]
    assert lib.dpvo_ba_max_free_poses() == 8192
    assert lib.dpvo_ba_set_marks(0) == 0
    for P, N in ((1, 7), (20, 7), (3, 17)):  # P < 2, P * P > 64, N > 16
        assert lib.dpvo_ba_plan_supported(256, 1, 1 + N, P) == 0
    assert lib.dpvo_ba_plan_supported(20000, 1, 8, 3) == 0

    f = lib.dpvo_ba_build_schur
    assert f(*ba, 0, 3, 4, 1, 8, one, None, None, None) == 0
    assert f(*ba, 256, 1, 4, 1, 8, one, None, None, None) == 1     # P
    assert f(*ba, 256, 3, 4, 8, 1, one, None, None, None) == 1     # t1 < t0
    assert f(*ba, 256, 3, 4, 1, 8, None, None, None, None) == 1    # workspace
    assert f(*ba, 256, 3, 4, 0, 21, one, None, None, None) == 3    # N > 20
    assert f(*ba, 20000, 3, 4, 1, 8, one, None, None, None) == 3   # E > 16384
    assert f(*ba, 20000, 1, 4, 1, 8, one, None, None, None) == 1   # INVALID before UNSUPPORTED
    f = lib.dpvo_ba_solve_update
    assert f(one, one, None, None, 0, 3, 4, 1, 8, one, None, None) == 0
    assert f(one, one, None, None, 256, 1, 4, 1, 8, one, None, None) == 1
    assert f(one, one, None, None, 256, 3, 4, 1, 8, None, None, None) == 1
    assert f(one, one, None, None, 256, 3, 4, 0, 21, one, None, None) == 3
    for f in (lib.dpvo_ba_last_status, lib.dpvo_ba_phase_marks, lib.dpvo_ba_workgroup_marks):
        assert f(None, 256, 1, 8, one, None) == 1
        assert f(one, 256, 1, 8, None, None) == 1
        assert f(one, 0, 1, 8, one, None) == 1
    f = lib.dpvo_ba_last_dx
    assert f(None, 256, 1, 8, one, None) == 1
    assert f(one, 256, 8, 1, one, None) == 1
    assert f(one, 0, 1, 8, one, None) == 1
    assert f(one, 256, 4, 4, one, None) == 0  # N == 0: nothing to copy
    f = lib.dpvo_ba_status_accumulate
    assert f(None, 256, 1, 8, one, None) == 1
    assert f(one, 256, 1, 8, None, None) == 1
    assert f(one, 0, 1, 8, one, None) == 0
    assert f(None, 0, 1, 8, one, None) == 1  # INVALID before the E <= 0 no-op here

    f = lib.dpvo_ba_plan_offsets
    assert f(0, 1, 8, out5) == 1
    assert f(256, 8, 1, out5) == 1
    assert f(256, 1, 8, None) == 1
    assert f(20000, 1, 8, out5) == 3
    f = lib.dpvo_ba_plan
    assert f(None, None, None, 0, 0, 0, 8, 1, None, small, None) == 0
    assert f(one, one, one, 256, 100, 9, 8, 1, one, big, None) == 1
    assert f(None, one, one, 256, 100, 9, 1, 8, one, big, None) == 1
    assert f(one, one, one, 256, 0, 9, 1, 8, one, big, None) == 1
    assert f(one, one, one, 20000, 100, 9, 8, 1, one, small, None) == 1  # INVALID first
    assert f(one, one, one, 20000, 100, 9, 1, 8, one, small, None) == 3  # UNSUPPORTED before WORKSPACE
    assert f(one, one, one, 256, 100, 9, 1, 8, one, small, None) == declined

    f = lib.dpvo_ba_forward  # .., E, P, num_poses, num_patches, PPF, t0, t1, iterations, eff_impl
    assert f(*(None,) * 9, 0, 3, 9, 100, 0, 1, 8, 2, 0, None, small, None) == 0
    assert f(*ba, 256, 3, 9, 100, 0, 1, 8, 0, 0, one, big, None) == 0      # no iterations
    assert f(*ba, 256, 1, 9, 100, 0, 1, 8, 2, 0, one, big, None) == 1      # P
    assert f(*ba, 256, 3, 9, 100, 0, 8, 1, 2, 0, one, big, None) == 1      # t1 < t0
    assert f(*ba[:8], None, 256, 3, 9, 100, 0, 1, 8, 2, 0, one, big, None) == 1  # kk
    assert f(*ba, 256, 3, 9, 100, 0, 1, 8, 2, 0, one, small, None) == 4
    assert f(*ba, 256, 1, 9, 100, 0, 1, 8, 2, 0, one, small, None) == 1    # INVALID before WORKSPACE
    assert f(*ba, 20000, 3, 9, 100, 0, 1, 8, 2, 0, one, small, None) == 4  # large graph alike
    f = lib.dpvo_ba_forward_planned  # .., E, P, num_poses, num_patches, t0, t1, iterations
    assert f(*(None,) * 9, 0, 3, 9, 100, 1, 8, 2, None, small, None) == 0
    assert f(*ba, 256, 3, 9, 100, 1, 8, 0, one, big, None) == 0
    assert f(*ba, 256, 1, 9, 100, 1, 8, 2, one, big, None) == 1
    assert f(*ba, 256, 3, 9, 100, 8, 1, 2, one, big, None) == 1
    assert f(*ba, 256, 3, 9, 100, 1, 8, 2, None, big, None) == 1
    assert f(*ba, 20000, 3, 9, 100, 1, 8, 2, one, small, None) == 3
    assert f(*ba, 256, 20, 9, 100, 1, 8, 2, one, small, None) == 3  # P * P > 64
    assert f(*ba, 256, 3, 9, 100, 1, 8, 2, one, small, None) == declined
    f = lib.dpvo_ba_forward_planned_dev  # .., num_patches, t0_dev, N, iterations
    assert f(*(None,) * 9, 0, 3, 9, 100, None, 7, 2, None, small, None) == 0
    assert f(*ba, 256, 1, 9, 100, one, 7, 2, one, big, None) == 1
    assert f(*ba, 256, 3, 9, 100, None, 7, 2, one, big, None) == 1   # t0_dev
    assert f(*ba, 256, 3, 9, 100, one, -1, 2, one, big, None) == 1   # N < 0
    assert f(*ba, 256, 3, 9, 100, one, 17, 2, one, small, None) == 3
    assert f(*ba, 256, 3, 9, 100, one, 7, 2, one, small, None) == declined

    f = lib.dpvo_reproject  # .., E, P, num_poses, num_patches, coords
    assert f(*edges, 0, 3, 9, 100, one, None) == 0
    assert f(*edges, 256, 0, 9, 100, one, None) == 1
    assert f(*edges, 256, 3, 0, 100, one, None) == 1
    f = lib.dpvo_reproject_ordered  # .., num_patches, N2, coords, order
    assert f(*edges, 0, 3, 9, 100, 9, one, one, None) == 0
    assert f(*edges, 256, 3, 9, 0, 9, one, one, None) == 1
    assert f(*edges, 256, 3, 9, 100, 9, one, None, None) == 1
    f = lib.dpvo_reproject_ordered_plan  # .., N2, coords, order, t0, t1, workspace, bytes
    assert f(*(None,) * 6, 0, 3, 9, 100, 9, None, None, 1, 8, None, small, None) == 0
    assert f(*edges, 256, 3, 9, 100, 9, one, None, 1, 8, one, big, None) == 1
    assert f(*edges, 256, 3, 9, 100, 9, one, one, 8, 1, one, big, None) == 1
    assert f(*edges, 20000, 3, 9, 100, 9, one, one, 1, 8, one, small, None) == 3
    assert f(*edges, 256, 3, 9, 100, 9, one, one, 1, 8, one, small, None) == declined
    f = lib.dpvo_reproject_ordered_plan_dev  # .., order, t0_dev, N, workspace, bytes
    assert f(*(None,) * 6, 0, 3, 9, 100, 9, None, None, None, 7, None, small, None) == 0
    assert f(*edges, 256, 3, 9, 100, 9, one, one, None, 7, one, big, None) == 1
    assert f(*edges, 256, 3, 9, 100, 9, one, one, one, -1, one, big, None) == 1
    assert f(*edges, 256, 3, 9, 100, 9, one, one, one, 17, one, small, None) == 3
    assert f(*edges, 256, 3, 9, 100, 9, one, one, one, 7, one, small, None) == declined

    # .., workspace, bytes, src, dst, scale, L, C, H, W, dtype; dst / scale are read on the host
    f = lib.dpvo_reproject_ordered_plan_insert
    dst, scale = (ctypes.c_void_p * 2)(1, 1), (ctypes.c_int * 2)(1, 4)
    head = (*edges, 256, 3, 9, 100, 9, one, one, 1, 8, one, small)
    assert f(*(None,) * 6, 0, 3, 9, 100, 9, None, None, 1, 8, None, small, None, None, None, 0, 0,
             0, 0, 0, None) == 0
    assert f(*head, None, dst, scale, 2, 64, 32, 32, 0, None) == 1       # src
    assert f(*head, one, dst, scale, 0, 64, 32, 32, 0, None) == 1        # L
    assert f(*head, one, dst, scale, 2, 64, 32, 32, 2, None) == 3        # fp64 pyramid
    assert f(*head, one, dst, scale, 5, 64, 32, 32, 0, None) == 3        # L > 4
    assert f(*head, one, (ctypes.c_void_p * 2)(1, None), scale, 2, 64, 32, 32, 0, None) == 1
    assert f(*head, one, dst, (ctypes.c_int * 2)(1, 3), 2, 64, 32, 32, 0, None) == 3
    assert f(*head[:6], 20000, *head[7:], one, dst, scale, 2, 64, 32, 32, 0, None) == 3
    assert f(*head, one, dst, scale, 2, 64, 32, 32, 1, None) == declined


def _levels(L, fmap2=1, H2=8, W2=8, scale=1.0, at=0):
    """Host level arrays (fmap2, H2, W2, scale) of L good levels; a keyword
    replaces the value of level `at`."""
    f = (ctypes.c_void_p * max(L, 1))(*[1] * L)
    h = (ctypes.c_int * max(L, 1))(*[8] * L)
    w = (ctypes.c_int * max(L, 1))(*[8] * L)
    s = (ctypes.c_float * max(L, 1))(*[1.0] * L)
    if L > 0:
        f[at], h[at], w[at], s[at] = fmap2, H2, W2, scale
    return f, h, w, s


def test_corr_return_codes(lib):
    """Return code of every dpvo_corr_* / dpvo_patchify_* / dpvo_feature_*
    export, and which check wins where two apply.  Every row is answered on
    the host before any launch or memset (the device pointers are dummies; the
    level arrays are real host arrays, the entries read them).  The literals
    of the first block were recorded from the build before the A-CORR host
    layer was refactored; the second block holds the checks that refactor
    added."""
    one, nan = ctypes.c_void_p(1), float("nan")
    OK, INVALID, UNSUPPORTED = 0, 1, 3
    p5 = (one,) * 5

    # ---- dpvo_corr_forward: fmap1, fmap2, coords, ii, jj, B, M, C, H, W, N1, N2, H2, W2,
    #      radius, dtype, out
    f = lib.dpvo_corr_forward
    for B, M, C, H, W, H2, W2, R in ((-1, 4, 128, 3, 3, 8, 8, 3), (1, -4, 128, 3, 3, 8, 8, 3),
                                     (1, 4, 0, 3, 3, 8, 8, 3), (1, 4, 128, 0, 3, 8, 8, 3),
                                     (1, 4, 128, 3, 0, 8, 8, 3), (1, 4, 128, 3, 3, 0, 8, 3),
                                     (1, 4, 128, 3, 3, 8, 0, 3), (1, 4, 128, 3, 3, 8, 8, -1),
                                     (1, 4, 128, 3, 3, 8, 8, 8)):
        assert f(*p5, B, M, C, H, W, 9, 4, H2, W2, R, 0, one, None) == INVALID
    for k in range(5):  # each null input with work to do
        p = p5[:k] + (None,) + p5[k + 1:]
        assert f(*p, 1, 4, 128, 3, 3, 9, 4, 8, 8, 3, 0, one, None) == INVALID
    assert f(*p5, 1, 4, 128, 3, 3, 9, 4, 8, 8, 3, 0, None, None) == INVALID      # out
    assert f(*p5, 1, 4, 128, 3, 3, 9, 4, 8, 8, 3, 7, one, None) == INVALID       # unknown dtype
    assert f(*p5, 1, 4, 128, 5, 4, 9, 4, 8, 8, 3, 0, one, None) == UNSUPPORTED   # H * W > 16
    assert f(*p5, 0, 4, 128, 3, 3, 9, 4, 8, 8, 3, 0, one, None) == OK
    assert f(*p5, 1, 0, 128, 3, 3, 9, 4, 8, 8, 3, 1, one, None) == OK
    # two checks
    assert f(*p5, 1, 4, 128, 5, 5, 9, 4, 8, 8, 8, 0, one, None) == INVALID       # radius, H * W
    assert f(*p5, 1, 0, 128, 5, 5, 9, 4, 8, 8, 3, 0, one, None) == UNSUPPORTED   # H * W, no work
    assert f(*p5, 1, 0, 128, 3, 3, 9, 4, 0, 8, 3, 0, one, None) == INVALID       # H2, no work
    assert f(*(None,) * 5, 1, 4, 128, 5, 5, 9, 4, 8, 8, 3, 0, None, None) == UNSUPPORTED
    assert f(*(None,) * 5, 1, 0, 128, 3, 3, 9, 4, 8, 8, 3, 0, None, None) == OK  # null, no work
    assert f(*p5, 1, 4, 128, 5, 5, 9, 4, 8, 8, 3, 7, one, None) == UNSUPPORTED   # dtype, H * W
    assert f(*p5, 1, 0, 128, 3, 3, 9, 4, 8, 8, 3, 7, one, None) == OK            # dtype, no work
    assert f(None, *p5[1:], 1, 4, 128, 3, 3, 9, 4, 8, 8, 3, 7, one, None) == INVALID

    # ---- dpvo_corr_forward_levels: fmap1, fmap2[], H2[], W2[], scale[], L, coords, ii, jj,
    #      B, M, C, H, W, N1, N2, radius, dtype, out
    f = lib.dpvo_corr_forward_levels
    good = _levels(2)

    def lv(arrs, L, B=1, M=4, C=128, H=3, W=3, R=3, dtype=0):
        return lib.dpvo_corr_forward_levels(one, *arrs, L, one, one, one, B, M, C, H, W, 9, 4, R,
                                            dtype, one, None)

    assert lv(good, 0) == INVALID and lv(_levels(8), 9) == INVALID
    assert lv(good, 2, R=-1) == INVALID and lv(good, 2, R=8) == INVALID
    assert lv(good, 2, C=0) == INVALID and lv(good, 2, H=0) == INVALID
    assert lv(good, 2, W=0) == INVALID
    for bad in (dict(fmap2=None), dict(H2=0), dict(W2=-3), dict(scale=0.0), dict(scale=nan)):
        assert lv(_levels(2, at=1, **bad), 2) == INVALID
    assert lv(good, 2, H=5, W=4) == UNSUPPORTED
    assert lv(good, 2, dtype=2) == UNSUPPORTED        # fp64: the single-level entry only
    assert lv(good, 2, dtype=7) == UNSUPPORTED
    assert lv(good, 2, M=0) == OK and lv(good, 2, B=0) == OK
    assert lv(_levels(8), 8, M=0) == OK               # the VALU entry takes 8 levels
    # two checks
    assert lv(_levels(8), 9, H=5, W=5) == INVALID                    # L, H * W
    assert lv(good, 2, H=5, W=5, M=0) == UNSUPPORTED                 # H * W, no work
    assert lv(_levels(2, H2=0), 2, M=0) == OK                        # level, no work
    assert lv(_levels(2, H2=0), 2, H=5, W=5) == UNSUPPORTED          # level, H * W
    assert lv(_levels(2, scale=-1.0), 2, dtype=2) == INVALID         # level, dtype
    assert lv(good, 2, dtype=2, M=0) == OK                           # dtype, no work
    assert lv(good, 2, dtype=2, H=5, W=5) == UNSUPPORTED

    # ---- dpvo_corr_forward_levels_nhwc[_ordered]: the same arguments (+ order before B)
    def entries():
        g = lib.dpvo_corr_forward_levels_nhwc

        def plain(ptrs, arrs, L, B=1, M=4, C=128, H=3, W=3, R=3, dtype=0, out=one):
            f1, co, ii, jj = ptrs
            return g(f1, *arrs, L, co, ii, jj, B, M, C, H, W, 9, 4, R, dtype, out, None)

        h = lib.dpvo_corr_forward_levels_nhwc_ordered

        def ordered(ptrs, arrs, L, B=1, M=4, C=128, H=3, W=3, R=3, dtype=0, out=one):
            f1, co, ii, jj = ptrs
            return h(f1, *arrs, L, co, ii, jj, one, B, M, C, H, W, 9, 4, R, dtype, out, None)

        return plain, ordered

    p4 = (one,) * 4
    for nh in entries():
        assert nh(p4, good, 0) == INVALID and nh(p4, good, -2) == INVALID
        assert nh(p4, good, 2, R=-1) == INVALID and nh(p4, good, 2, R=8) == INVALID
        assert nh(p4, good, 2, C=0) == INVALID and nh(p4, good, 2, H=0) == INVALID
        assert nh(p4, good, 2, W=0) == INVALID
        for k in range(4):  # each null input with work to do
            assert nh(p4[:k] + (None,) + p4[k + 1:], good, 2) == INVALID
        assert nh(p4, good, 2, out=None) == INVALID
        for bad in (dict(fmap2=None), dict(H2=0), dict(W2=-3), dict(scale=0.0), dict(scale=nan)):
            assert nh(p4, _levels(2, at=1, **bad), 2) == INVALID
        assert nh(p4, good, 2, dtype=2) == UNSUPPORTED and nh(p4, good, 2, dtype=7) == UNSUPPORTED
        assert nh(p4, good, 2, C=64) == UNSUPPORTED
        assert nh(p4, _levels(5), 5) == UNSUPPORTED                  # L > 4
        assert nh(p4, good, 2, H=5, W=4) == UNSUPPORTED              # H * W > 16
        assert nh(p4, good, 2, R=4) == UNSUPPORTED                   # 81 * 9 outputs > 512
        assert nh(p4, good, 2, H=1, W=1, R=6) == UNSUPPORTED         # D * D = 196 > 164
        assert nh(p4, good, 2, M=0) == OK and nh(p4, good, 2, B=0) == OK
        assert nh(p4, good, 2, M=0, dtype=1) == OK
        # two checks
        assert nh(p4, good, 0, C=64) == INVALID                      # L, C
        assert nh(p4, good, 2, C=64, M=0) == UNSUPPORTED             # C, no work
        assert nh(p4, _levels(2, H2=0), 2, M=0) == OK                # level, no work
        assert nh(p4, _levels(2, H2=0), 2, C=64) == UNSUPPORTED      # level, C
        assert nh(p4, _levels(2, H2=0), 2, H=1, W=1, R=6) == INVALID     # level, D * D
        assert nh(p4, good, 2, H=1, W=1, R=6, M=0) == OK             # D * D, no work
        assert nh(p4, _levels(8), 9, R=8) == INVALID                 # radius, L

    # ---- dpvo_corr_backward: .., jj, grad, B, M, C, H, W, N1, N2, H2, W2, radius, dtype, g1, g2
    # (rows rejected ahead of the memset of the gradients only)
    f = lib.dpvo_corr_backward
    p6 = (one,) * 6
    for B, M, C, H, W, R in ((-1, 4, 128, 3, 3, 3), (1, -4, 128, 3, 3, 3), (1, 4, 0, 3, 3, 3),
                             (1, 4, 128, 0, 3, 3), (1, 4, 128, 3, 0, 3), (1, 4, 128, 3, 3, -1),
                             (1, 4, 128, 3, 3, 8)):
        assert f(*p6, B, M, C, H, W, 9, 4, 8, 8, R, 0, one, one, None) == INVALID
    assert f(*p6, 1, 4, 128, 5, 4, 9, 4, 8, 8, 3, 0, one, one, None) == UNSUPPORTED
    assert f(*p6, 1, 4, 128, 3, 3, 9, 4, 8, 8, 3, 1, one, one, None) == UNSUPPORTED  # fp16
    assert f(*p6, 1, 4, 128, 3, 3, 9, 4, 8, 8, 3, 2, one, one, None) == UNSUPPORTED  # fp64
    assert f(*p6, 1, 4, 128, 5, 5, 9, 4, 8, 8, 8, 0, one, one, None) == INVALID      # radius, H * W
    assert f(*p6, 1, 4, 0, 3, 3, 9, 4, 8, 8, 3, 1, one, one, None) == INVALID        # C, dtype
    assert f(*p6, 1, 0, 128, 5, 5, 9, 4, 8, 8, 3, 1, one, one, None) == UNSUPPORTED

    # ---- dpvo_patchify_forward: net, coords, B, C, H, W, M, radius, clamp, dtype, out
    f = lib.dpvo_patchify_forward
    for B, C, H, W, M, R in ((-1, 8, 6, 6, 4, 3), (1, 0, 6, 6, 4, 3), (1, 8, 0, 6, 4, 3),
                             (1, 8, 6, 0, 4, 3), (1, 8, 6, 6, -4, 3), (1, 8, 6, 6, 4, -1)):
        assert f(one, one, B, C, H, W, M, R, 0, 0, one, None) == INVALID
    assert f(one, one, 1, 8, 6, 6, 4, 3, 0, 7, one, None) == INVALID      # unknown dtype
    assert f(one, one, 0, 8, 6, 6, 4, 3, 0, 0, one, None) == OK
    assert f(one, one, 1, 8, 6, 6, 0, 3, 1, 2, one, None) == OK
    assert f(one, one, 1, 8, 6, 6, 0, 3, 0, 7, one, None) == OK           # dtype, no work
    assert f(one, one, 1, 0, 6, 6, 0, 3, 0, 7, one, None) == INVALID      # C, no work
    # ---- dpvo_patchify_backward: grad, coords, .., net_grad (rows ahead of the memset only)
    f = lib.dpvo_patchify_backward
    for B, C, H, W, M, R in ((-1, 8, 6, 6, 4, 3), (1, 0, 6, 6, 4, 3), (1, 8, 0, 6, 4, 3),
                             (1, 8, 6, 0, 4, 3), (1, 8, 6, 6, -4, 3), (1, 8, 6, 6, 4, -1)):
        assert f(one, one, B, C, H, W, M, R, 0, 0, one, None) == INVALID
    assert f(one, one, 1, 8, 6, 6, 4, 3, 0, 1, one, None) == UNSUPPORTED
    assert f(one, one, 1, 8, 6, 6, 4, 3, 0, 2, one, None) == UNSUPPORTED
    assert f(one, one, 1, 0, 6, 6, 4, 3, 0, 1, one, None) == INVALID      # C, dtype
    assert f(one, one, 1, 8, 6, 6, 0, 3, 0, 1, one, None) == UNSUPPORTED  # dtype, no work

    # ---- dpvo_feature_to_nhwc: src, dst, count, C, H, W, dtype
    f = lib.dpvo_feature_to_nhwc
    for count, C, H, W in ((-1, 8, 6, 6), (2, 0, 6, 6), (2, 8, 0, 6), (2, 8, 6, 0)):
        assert f(one, one, count, C, H, W, 0, None) == INVALID
    assert f(None, one, 2, 8, 6, 6, 0, None) == INVALID and f(one, None, 2, 8, 6, 6, 0, None) == INVALID
    assert f(one, one, 2, 8, 6, 6, 2, None) == UNSUPPORTED and f(one, one, 2, 8, 6, 6, 7, None) == UNSUPPORTED
    assert f(one, one, 0, 8, 6, 6, 0, None) == OK
    assert f(one, one, 0, 8, 6, 6, 2, None) == OK          # dtype, no work
    assert f(None, one, 0, 8, 6, 6, 0, None) == INVALID    # null, no work
    assert f(None, one, 2, 8, 6, 6, 2, None) == INVALID    # null, dtype

    # ---- dpvo_feature_pyramid_insert: src, dst[], scale[], L, C, H, W, dtype
    f = lib.dpvo_feature_pyramid_insert
    VP, I4, I8 = ctypes.c_void_p * 2, ctypes.c_int * 2, ctypes.c_int64 * 2
    dst, scale = VP(1, 1), I4(1, 4)
    assert f(None, dst, scale, 2, 64, 32, 32, 0, None) == INVALID
    assert f(one, None, scale, 2, 64, 32, 32, 0, None) == INVALID
    assert f(one, dst, None, 2, 64, 32, 32, 0, None) == INVALID
    assert f(one, dst, scale, 0, 64, 32, 32, 0, None) == INVALID
    for C, H, W in ((0, 32, 32), (64, 0, 32), (64, 32, 0)):
        assert f(one, dst, scale, 2, C, H, W, 0, None) == INVALID
    assert f(one, VP(1, None), scale, 2, 64, 32, 32, 1, None) == INVALID
    assert f(one, dst, scale, 2, 64, 32, 32, 2, None) == UNSUPPORTED      # fp64 pyramid
    assert f(one, dst, scale, 5, 64, 32, 32, 0, None) == UNSUPPORTED      # L > 4
    assert f(one, dst, I4(1, 3), 2, 64, 32, 32, 0, None) == UNSUPPORTED
    assert f(one, dst, I4(16, 1), 2, 64, 32, 32, 1, None) == UNSUPPORTED
    assert f(one, dst, scale, 0, 64, 32, 32, 2, None) == INVALID              # L, dtype
    assert f(one, VP(1, None), scale, 2, 64, 32, 32, 2, None) == UNSUPPORTED  # dtype, null level
    assert f(one, VP(None, 1), I4(1, 3), 2, 64, 32, 32, 0, None) == INVALID   # level 0 first
    assert f(one, VP(1, None), I4(3, 1), 2, 64, 32, 32, 0, None) == UNSUPPORTED
    # ---- dpvo_feature_pyramid_insert_ring: src, dst0[], slot_bytes[], scale[], L, C, H, W, mem,
    #      slot_dev, dtype
    f = lib.dpvo_feature_pyramid_insert_ring
    sb = I8(1 << 20, 1 << 16)
    assert f(one, dst, sb, scale, 2, 64, 32, 32, 8, None, 0, None) == INVALID   # slot_dev
    assert f(one, dst, sb, scale, 2, 64, 32, 32, 0, one, 0, None) == INVALID    # mem
    assert f(one, dst, None, scale, 2, 64, 32, 32, 8, one, 0, None) == INVALID  # slot_bytes
    assert f(None, dst, sb, scale, 2, 64, 32, 32, 8, one, 0, None) == INVALID
    assert f(one, dst, sb, scale, 0, 64, 32, 32, 8, one, 0, None) == INVALID
    assert f(one, VP(1, None), sb, scale, 2, 64, 32, 32, 8, one, 0, None) == INVALID
    assert f(one, dst, sb, scale, 2, 64, 32, 32, 8, one, 2, None) == UNSUPPORTED
    assert f(one, dst, sb, scale, 5, 64, 32, 32, 8, one, 1, None) == UNSUPPORTED
    assert f(one, dst, sb, I4(1, 5), 2, 64, 32, 32, 8, one, 0, None) == UNSUPPORTED
    assert f(one, dst, sb, scale, 2, 64, 32, 32, 8, None, 2, None) == INVALID       # slot_dev, dtype
    assert f(one, dst, sb, scale, 2, 64, 32, 32, 0, one, 2, None) == UNSUPPORTED    # mem, dtype
    assert f(one, dst, None, I4(1, 3), 2, 64, 32, 32, 8, one, 0, None) == INVALID   # slot_bytes, scale

    # ==== The rows below differ from the build before the refactor: the checks
    # ==== it added (dpvo_corr_forward_levels and the channels-last entries now
    # ==== look at B, M and every pointer first), and the new query export.
    if not hasattr(lib, "dpvo_corr_query_path"):
        pytest.fail("dpvo_corr_query_path is not exported")
    f = lib.dpvo_corr_forward_levels
    assert lv(good, 2, B=-1) == INVALID and lv(good, 2, M=-4) == INVALID
    assert lv(good, 2, B=-1, M=-4) == INVALID                        # B * M > 0 reached the launch
    for k in range(4):  # fmap2 / H2 / W2 / scale arrays
        assert lv(good[:k] + (None,) + good[k + 1:], 2) == INVALID
        assert lv(good[:k] + (None,) + good[k + 1:], 2, M=0) == INVALID
    for k in (0, 6, 7, 8, 18):  # fmap1, coords, ii, jj, out
        a = [one, *good, 2, one, one, one, 1, 4, 128, 3, 3, 9, 4, 3, 0, one, None]
        a[k] = None
        assert f(*a) == INVALID
        a[10] = 0  # M
        assert f(*a) == INVALID
        a[12], a[13] = 5, 5
        assert f(*a) == INVALID                                      # null before H * W
    for nh in entries():
        assert nh(p4, good, 2, B=-1) == INVALID and nh(p4, good, 2, M=-4) == INVALID
        for k in range(4):
            arrs = good[:k] + (None,) + good[k + 1:]
            assert nh(p4, arrs, 2) == INVALID and nh(p4, arrs, 2, M=0) == INVALID
            ptrs = p4[:k] + (None,) + p4[k + 1:]
            assert nh(ptrs, good, 2, M=0) == INVALID
            assert nh(ptrs, good, 2, C=64) == INVALID                # null before the envelope
        assert nh(p4, good, 2, M=0, out=None) == INVALID
    # dpvo_corr_query_path: entry, then the ordered entry's arguments without stream; path out
    q = lib.dpvo_corr_query_path
    path = ctypes.c_int(-1)

    def query(entry, arrs, L, B=1, M=4, C=128, H=3, W=3, N2=4, R=3, dtype=0, f1=16):
        path.value = -1
        st = q(entry, ctypes.c_void_p(f1), *arrs, L, one, one, one, None, B, M, C, H, W, 9, N2, R,
               dtype, one, ctypes.byref(path))
        return st, path.value

    NONE, NHWC, MMA, MMA_ORDERED, VALU = range(5)
    al = _levels(2, fmap2=16)
    al[0][1] = 16
    assert query(0, al, 1) == (OK, MMA) and query(1, al, 2) == (OK, MMA)
    assert query(2, al, 2) == (OK, NHWC)
    assert query(0, al, 1, C=64) == (OK, VALU) and query(1, al, 2, f1=8) == (OK, VALU)
    assert query(0, al, 1, dtype=2) == (OK, VALU)
    assert query(1, al, 2, dtype=2) == (UNSUPPORTED, NONE)
    assert query(0, al, 1, dtype=7) == (INVALID, NONE)
    assert query(2, al, 2, C=64) == (UNSUPPORTED, NONE)
    assert query(1, al, 2, M=0) == (OK, NONE)
    assert query(3, al, 2) == (INVALID, NONE)                        # no such entry
    assert q(1, one, *al, 2, one, one, one, None, 1, 4, 128, 3, 3, 9, 4, 3, 0, one, None) == INVALID
    big = _levels(1, fmap2=16, H2=128, W2=128)                       # 1100 x 128 x 128^2 x 4 B
    assert query(1, big, 1, N2=1100) == (OK, MMA_ORDERED)
    assert query(1, big, 1, N2=1100, B=2) == (OK, MMA)


def test_workspace_size_grows_with_problem(lib):
    a = lib.dpvo_ba_workspace_bytes(256, 1, 8)
    b = lib.dpvo_ba_workspace_bytes(2048, 1, 12)
    assert 0 < a < b


def test_extension_modules_expose_reference_surface():
    import dpvo_amd

    corr = dpvo_amd.load_extension("cuda_corr")
    ba = dpvo_amd.load_extension("cuda_ba")
    lie = dpvo_amd.load_extension("lietorch_backends")
    for n in ["forward", "backward", "patchify_forward", "patchify_backward"]:
        assert hasattr(corr, n)  # correlation.cpp:57-63
    for n in ["forward", "neighbors", "reproject", "solve_system"]:
        assert hasattr(ba, n)  # ba.cpp:183-189
    for n in ["expm", "expm_backward", "logm", "logm_backward", "inv", "inv_backward", "mul",
              "mul_backward", "adj", "adj_backward", "adjT", "adjT_backward", "act",
              "act_backward", "act4", "act4_backward", "as_matrix", "projector", "Jinv"]:
        assert hasattr(lie, n)  # lietorch.cpp:286-316
    # the import is the in-tree build, not something on site-packages
    assert os.path.realpath(corr.__file__).startswith(os.path.realpath(dpvo_amd.NATIVE_DIR))


def test_cpu_tensors_are_rejected_loudly():
    import torch

    import dpvo_amd

    corr = dpvo_amd.load_extension("cuda_corr")
    f1 = torch.zeros(1, 2, 8, 3, 3)
    f2 = torch.zeros(1, 2, 8, 10, 10)
    co = torch.zeros(1, 1, 2, 3, 3)
    ii = torch.zeros(1, dtype=torch.long)
    with pytest.raises(RuntimeError, match="GPU"):
        corr.forward(f1, f2, co, ii, ii, 3)


def _cpu_calls():
    """module -> {entry: call with CPU tensors of the right dtype and shape in
    every tensor slot}: 4 poses, 6 patches of 3 x 3, 8 edges, window (1, 4)."""
    import torch

    def f(*s):
        return torch.zeros(*s)

    def d(*s):
        return torch.zeros(*s, dtype=torch.float64)

    def l(*s):
        return torch.zeros(*s, dtype=torch.long)

    def i(*s):
        return torch.zeros(*s, dtype=torch.int32)

    def u8(*s):
        return torch.zeros(*s, dtype=torch.uint8)

    poses, patches, intr = f(4, 7), f(6, 3, 3, 3), f(4, 4)
    ii, jj, kk = l(8), l(8), l(8)
    tgt, wgt, lm = f(8, 2), f(8, 2), f(1)
    edge = (poses, patches, intr, ii, jj, kk)
    ba = (poses, patches, intr, tgt, wgt, lm, ii, jj, kk)
    ws, t0_dev = u8(64), i(1)
    src, dst = f(8, 8, 8), [f(8, 8, 8).permute(2, 0, 1), f(4, 4, 8).permute(2, 0, 1)]
    # the patch-graph store: max_edges 16, DIM 16, counts of 3 words
    live = [l(16), l(16), l(16), f(16, 16)]
    act, back = live + [f(16, 2), f(16, 2)], [l(16), l(16), l(16), f(16, 16), f(16, 2), f(16, 2)]
    inac = [l(16), l(16), l(16), f(16, 2), f(16, 2)]
    counts, pos, ix, st, kf, mag = i(3), i(16), l(6), i(1), i(2), f(2)
    coords = f(8, 3, 3, 2)
    disps, images = f(4, 6, 8), f(4, 3, 6, 8)
    kps = f(5, 2)
    cuda_ba = {
        "forward": lambda m: m.forward(*ba, 1, 1, 4, 2, False),
        "forward_dx": lambda m: m.forward_dx(*ba, 1, 1, 4, 2, False),
        "forward_marks": lambda m: m.forward_marks(*ba, 1, 1, 4, 2, False),
        "forward_planned": lambda m: m.forward_planned(ws, *ba, 1, 4, 2),
        "forward_planned_dev": lambda m: m.forward_planned_dev(ws, *ba, t0_dev, 3, 2),
        "reproject": lambda m: m.reproject(*edge),
        "reproject_ordered": lambda m: m.reproject_ordered(*edge, 4),
        "reproject_ordered_plan": lambda m: m.reproject_ordered_plan(*edge, 4, 1, 4),
        "reproject_ordered_plan_dev": lambda m: m.reproject_ordered_plan_dev(*edge, 4, t0_dev, 3),
        "reproject_ordered_plan_insert": lambda m: m.reproject_ordered_plan_insert(
            *edge, 4, 1, 4, src, dst, [1, 2]),
        "neighbors": lambda m: m.neighbors(ii, jj),
        "pgo_residual": lambda m: m.pgo_residual(f(5, 7), f(3, 8), l(3), l(3), True),
        "ransac_umeyama": lambda m: m.ransac_umeyama(f(20, 3), f(20, 3), i(2, 3), 0.1, 100),
        "setup": lambda m: m.setup(ii, jj, kk, 6, 1, 4),
        "plan": lambda m: m.plan(ii, jj, kk, 6, 4, 1, 4),
        "build_schur": lambda m: m.build_schur(ws, *ba, 1, 4),
        "solve_update": lambda m: m.solve_update(ws, poses, patches, d(6, 6, 6), d(18), 8, 1, 4),
        "last_status": lambda m: m.last_status(ws, 8, 1, 4),
        "check_status": lambda m: m.check_status(f(1)),
        "gba_setup": lambda m: m.gba_setup(ii, jj, kk, 6, 1, 1, 4, 0, 6),
        "gba_build": lambda m: m.gba_build(ws, poses, patches, intr, tgt, wgt, lm, ii, jj, 1, 4),
        "gba_packed": lambda m: m.gba_packed(ws, 8, 1, 4, 1),
        "gba_solve_update": lambda m: m.gba_solve_update(ws, poses, patches, 8, 1, 4),
        "gba_info": lambda m: m.gba_info(ws, 8, 1, 4),
        "workspace_marks": lambda m: m.workspace_marks(ws, 8, 1, 4),
        "last_dx": lambda m: m.last_dx(ws, 8, 1, 4),
        "spd_solve": lambda m: m.spd_solve(f(2, 3, 3), f(2, 3, 1)),
        "spd_solve_factored": lambda m: m.spd_solve_factored(f(2, 3, 3), f(2, 3, 1)),
        "pg_append": lambda m: m.pg_append(ix, l(4), l(4), *live, counts),
        "pg_append_dev": lambda m: m.pg_append_dev(ix, l(4), l(4), i(1), *live, counts),
        "pg_remove": lambda m: m.pg_remove(torch.zeros(16, dtype=torch.bool), ix, 0, 0, False, act,
                                           back, inac, counts, pos),
        "pg_remove_window_dev": lambda m: m.pg_remove_window_dev(ix, i(1), 0, 0, False, False, act,
                                                                 back, inac, counts, pos),
        "pg_remove_frame_dev": lambda m: m.pg_remove_frame_dev(kf, act, back, counts, pos),
        "kf_motion": lambda m: m.kf_motion(*live[:3], counts, poses, patches, intr, st, 4, 12.5, kf,
                                           mag),
        "kf_shift": lambda m: m.kf_shift(kf, 1, st, *live[:3], counts, [poses, intr], [0, 0], poses,
                                         l(4), f(8, 7), l(8), i(1)),
        "edges_loop": lambda m: m.edges_loop(poses, patches, intr, ix, 1, st, 4, i(1), 20, 1000, 15,
                                             4, 64.0, 4, 1, f(m.edges_loop_work_floats()), l(4),
                                             l(4), i(1), i(1)),
        "ba_layer_forward": lambda m: m.ba_layer_forward(poses, patches, intr, tgt, wgt, f(1), 1e-4,
                                                         ii, jj, kk, 4, 1, False,
                                                         [0.0, 0.0, 8.0, 8.0], 0.1, True),
        "ba_layer_backward": lambda m: m.ba_layer_backward(ws, *edge, f(3, 6), f(6), 4, 1, False),
        "transform_forward": lambda m: m.transform_forward(*edge, False),
        "transform_backward": lambda m: m.transform_backward(*edge, coords, True, True),
        "flow_loss_forward": lambda m: m.flow_loss_forward(coords, coords, f(8)),
        "flow_loss_backward": lambda m: m.flow_loss_backward(coords, coords, f(8), i(1), i(8), f(1)),
        "pose_loss_forward": lambda m: m.pose_loss_forward(poses, poses),
        "pose_loss_backward": lambda m: m.pose_loss_backward(poses, poses, f(2)),
        "frame_flow_distance": lambda m: m.frame_flow_distance(poses, disps, intr),
        "frame_graph": lambda m: m.frame_graph(f(4, 4)),
        "rgbd_augment": lambda m: m.rgbd_augment(images, disps, intr, 4, 4, False, [0, 1, 2, 3],
                                                 1.0, 1.0, 1.0, 0.0, False, False, 1.0, False),
        "normalize_depth": lambda m: m.normalize_depth(disps, poses),
        "frame_init": lambda m: m.frame_init(poses, f(8, 3, 3, 3), intr, l(4), d(10), f(2, 3, 3, 3),
                                             f(4), 2, 0, i(1), 0, i(1), 0, 0.5, 4.0, False),
        "trajectory": lambda m: m.trajectory(poses, l(4), 4, i(1), f(8, 7), l(8, 2), i(1), 5, False),
        "frame_prepare": lambda m: m.frame_prepare(u8(8, 8, 3), [4.0, 4.0, 4.0, 4.0], 1.0, False,
                                                   u8(3, 8, 8)),
        "trajectory_ate": lambda m: m.trajectory_ate(d(5, 3), d(5), d(6, 3), d(6)),
        "frame_sample": lambda m: m.frame_sample(f(8, 4, 4), f(16, 4, 4), f(3, 16, 16), f(2, 2),
                                                 f(3, 2, 8, 3, 3), f(3, 2, 16), f(2, 3, 3, 3),
                                                 u8(4, 2, 3), 4, 0, i(1)),
        "probe_median": lambda m: m.probe_median(f(6, 2)),
        "update_targets": lambda m: m.update_targets(f(1, 8, 2, 3, 3), f(8, 2), f(8, 2), tgt, wgt,
                                                     8, i(1)),
        "map_points": lambda m: m.map_points(poses, patches, intr, ix, f(6, 3), 6, i(1)),
        "match_descriptors": lambda m: m.match_descriptors(f(5, 8), f(6, 8), 0.8, 1.0, 5, i(1), 6,
                                                           i(1)),
        "triangulate_tracks": lambda m: m.triangulate_tracks(f(3, 7), f(3, 4), f(6), kps, kps, kps,
                                                             l(5), l(5), 10.0, 1.0, 2, 1e-3),
    }
    # Update: corr_dim 4, 8 edges; its 50 parameter tensors by element count
    K0 = 4
    up = [f(384 * K0 if k == 38 else 2 * 384 if k >= 46 else 384 * 384)
          if (k % 2 == 0 and k not in (8, 22, 30, 42)) else f(2 if k in (47, 49) else 384)
          for k in range(50)]
    net, corr = f(8, 384), f(8, K0)
    dpvo_update = {
        "plan": lambda m: m.plan(l(8), l(8), ws),
        "forward": lambda m: m.forward(ws, m.F32, net, net, corr, ii, jj, ws, net, tgt, wgt),
        "pack_weights_device": lambda m: m.pack_weights_device(up, K0, m.F32, ws),
        "forward_train": lambda m: m.forward_train(ws, net, net, corr, ii, jj, ws, ws, net, tgt,
                                                   wgt),
        "relu_masks": lambda m: m.relu_masks(ws, 8, K0),
        "backward": lambda m: m.backward(up, ws, ii, jj, K0, net, tgt, wgt, net, net, corr, up, ws),
    }
    # BasicEncoder4: output dim 64, one 8 x 8 image
    shape = [(32, 3, 7)] + [(32, 32, 3)] * 4 + [(64, 32, 3), (64, 64, 3), (64, 32, 1), (64, 64, 3),
                                                (64, 64, 3), (64, 64, 1)]
    ep = [f(s[0]) if k % 2 else f(s[0], s[1], s[2], s[2]) for s in shape for k in (0, 1)]
    img, out = f(1, 3, 8, 8), f(1, 64, 2, 2)
    dpvo_encoder = {
        "forward": lambda m: m.forward(ws, m.F32, m.NORM_NONE, img, out, ws),
        "pack_weights_device": lambda m: m.pack_weights_device(ep, 64, m.NORM_NONE, m.F32, ws),
        "forward_train": lambda m: m.forward_train(ws, m.F32, m.NORM_NONE, img, out, ws),
        "backward": lambda m: m.backward(m.NORM_NONE, ep, img, ws, out, ep, ws),
    }
    return {"cuda_ba": cuda_ba, "dpvo_update": dpvo_update, "dpvo_encoder": dpvo_encoder}


# CPU tensors by contract: the host packers, and solve_system (the loop-closure
# worker hands it CPU tensors, which it moves to the device itself)
_CPU_BY_CONTRACT = {"pack_weights", "solve_system"}


@pytest.mark.parametrize("module", ["cuda_ba", "dpvo_update", "dpvo_encoder"])
def test_cpu_tensors_are_rejected_by_every_entry(module):
    """Every entry that takes a device tensor refuses CPU tensors with its own
    message, before it builds a device guard from one of them (which dies
    with torch's INTERNAL ASSERT instead) and before any launch."""
    import dpvo_amd

    m = dpvo_amd.load_extension(module)
    calls = _cpu_calls()[module]
    takes_tensors = {n for n in dir(m) if callable(getattr(m, n)) and not n.startswith("_")
                     and "Tensor" in getattr(m, n).__doc__.split("\n")[0].rsplit("->", 1)[0]}
    assert set(calls) == takes_tensors - _CPU_BY_CONTRACT
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="GPU") as exc:
            call(m)
        assert "INTERNAL ASSERT" not in str(exc.value), name
