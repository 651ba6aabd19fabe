"""CPU: host-side validation of the front-end entry points of the C ABI
(dpvo_frame_init, dpvo_trajectory), before any launch -- no GPU needed."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    vp, i, d, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    lib.dpvo_frame_init.argtypes = [vp, vp, vp, vp, vp, i, vp, vp, i, i, i, i, vp, i, vp, i, d, d,
                                    i, vp]
    lib.dpvo_trajectory.argtypes = [vp, vp, i, i, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, sz, vp]
    lib.dpvo_trajectory_workspace_bytes.argtypes = [i]
    return lib


ONE = ctypes.c_void_p(1)  # a non-null pointer that is never dereferenced on the host


def _frame_init(lib, ptrs=None, N=8, M=4, P=3, n=2, n_dev=None, counter=2, counter_dev=None,
                times_cap=16, model=1, median=1, res=4.0):
    p = [ONE] * 7 if ptrs is None else ptrs
    return lib.dpvo_frame_init(p[0], p[1], p[2], p[3], p[4], times_cap, p[5], p[6], N, M, P, n,
                               n_dev, counter, counter_dev, model, 0.5, res, median, None)


def test_frame_init_null_pointers(lib):
    for k in range(7):
        ptrs = [ONE] * 7
        ptrs[k] = None
        assert _frame_init(lib, ptrs) == 1, k


def test_frame_init_bad_sizes(lib):
    assert _frame_init(lib, M=0) == 1
    assert _frame_init(lib, P=0) == 1
    assert _frame_init(lib, N=0) == 1
    assert _frame_init(lib, P=-3) == 1


def test_frame_init_host_index_out_of_range(lib):
    assert _frame_init(lib, n=8) == 1
    assert _frame_init(lib, n=-1) == 1
    assert _frame_init(lib, counter=-1) == 1
    assert _frame_init(lib, counter=16) == 1
    assert _frame_init(lib, model=2) == 1
    assert _frame_init(lib, median=2) == 1
    assert _frame_init(lib, res=0.0) == 1


def test_frame_init_median_cap(lib):
    # the select counts in int: unsupported far above the 3 x 1024 x 9 values asked for
    assert _frame_init(lib, N=1, n=0, M=1 << 20, P=32) == 3


def _trajectory(lib, counter, ptrs=None, N=8, n=2, cap=4, ws_bytes=None):
    p = [ONE] * 9 if ptrs is None else ptrs
    wsb = lib.dpvo_trajectory_workspace_bytes(max(counter, 0)) if ws_bytes is None else ws_bytes
    return lib.dpvo_trajectory(p[0], p[1], N, n, None, p[2], p[3], p[4], cap, counter, 1, p[5],
                               p[6], p[7], p[8], wsb, None)


def test_trajectory_counter_zero_is_a_noop(lib):
    assert _trajectory(lib, 0) == 0
    assert _trajectory(lib, 0, ptrs=[None] * 9) == 0


def test_trajectory_validation(lib):
    assert _trajectory(lib, -1) == 1
    for k in (0, 1, 4, 5, 6, 7, 8):  # poses, tstamps, count, traj, root, info, workspace
        ptrs = [ONE] * 9
        ptrs[k] = None
        assert _trajectory(lib, 5, ptrs) == 1, k
    ptrs = [ONE] * 9
    ptrs[2] = None  # a log of capacity > 0 needs its buffers
    assert _trajectory(lib, 5, ptrs) == 1
    assert _trajectory(lib, 5, n=9) == 1
    assert _trajectory(lib, 5, N=0) == 1
    assert _trajectory(lib, 5, ws_bytes=16) == 4  # workspace too small


def test_cpu_tensors_are_rejected_loudly():
    import torch

    import dpvo_amd
    from dpvo_amd import frontend

    ext = dpvo_amd.load_extension("cuda_ba")
    assert hasattr(ext, "frame_init") and hasattr(ext, "trajectory")
    N, M, P = 4, 2, 3
    poses, patches = torch.zeros(N, 7), torch.zeros(N * M, 3, P, P)
    intr, ts = torch.zeros(N, 4), torch.zeros(N, dtype=torch.long)
    times, new, ni = torch.zeros(8, dtype=torch.float64), torch.zeros(M, 3, P, P), torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU"):
        frontend.init_frame(poses, patches, intr, ts, times, new, ni, 2, 2, M)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.frame_init(poses, patches, intr, ts, times, new, ni, M, 2, None, 2, None, 1, 0.5, 4.0,
                       True)
    delta = (torch.zeros(2, 7), torch.zeros(2, 2, dtype=torch.long),
             torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        frontend.trajectory(poses, ts, 2, delta, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.trajectory(poses, ts, 2, None, *delta, 4, True)


def test_trajectory_workspace_bytes(lib):
    sizes = [lib.dpvo_trajectory_workspace_bytes(c) for c in (0, 1, 2, 3, 70, 4096, 4097, 100000)]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] > sizes[0]
