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
