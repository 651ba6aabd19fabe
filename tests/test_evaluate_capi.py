"""CPU: host-side validation of dpvo_trajectory_ate of the C ABI, before any
launch -- no GPU needed."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, F16, F64 = 0, 1, 2
ONE = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    vp, i, d, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    lib.dpvo_trajectory_ate.argtypes = [vp, i, vp, i, vp, vp, i, d, i, vp, vp, vp, vp, vp, sz, vp]
    lib.dpvo_trajectory_ate_workspace_bytes.argtypes = [i, i]
    return lib


def _ate(lib, ptrs=None, dtype=F64, n=40, m=50, max_diff=0.01, align=1, ws_bytes=None):
    p = [ONE] * 9 if ptrs is None else ptrs  # est_xyz est_t ref_xyz ref_t stats model pairs status ws
    wsb = lib.dpvo_trajectory_ate_workspace_bytes(max(n, 1), max(m, 1)) if ws_bytes is None else ws_bytes
    return lib.dpvo_trajectory_ate(p[0], dtype, p[1], n, p[2], p[3], m, max_diff, align, p[4], p[5],
                                   p[6], p[7], p[8], wsb, None)


def test_null_pointers(lib):
    for k in range(9):
        ptrs = [ONE] * 9
        ptrs[k] = None
        assert _ate(lib, ptrs) == INVALID, k


def test_bad_arguments(lib):
    assert _ate(lib, n=0) == INVALID
    assert _ate(lib, m=0) == INVALID
    assert _ate(lib, n=-5) == INVALID
    assert _ate(lib, max_diff=-1e-3) == INVALID
    assert _ate(lib, max_diff=float("nan")) == INVALID
    assert _ate(lib, align=2) == INVALID
    assert _ate(lib, align=-1) == INVALID


def test_limits(lib):
    assert _ate(lib, dtype=F16) == UNSUPPORTED
    assert _ate(lib, dtype=7) == UNSUPPORTED
    assert _ate(lib, n=65537) == UNSUPPORTED
    assert _ate(lib, m=65537) == UNSUPPORTED
    assert _ate(lib, n=1 << 20, m=1 << 20) == UNSUPPORTED


def test_order_of_the_checks(lib):
    assert _ate(lib, n=0, dtype=F16) == INVALID
    assert _ate(lib, dtype=F16, ws_bytes=0) == UNSUPPORTED
    assert _ate(lib, n=65537, ws_bytes=0) == UNSUPPORTED
    assert _ate(lib, ws_bytes=8 * 40 - 1) == WORKSPACE
    assert _ate(lib, n=65536, m=65536, ws_bytes=8) == WORKSPACE


def test_workspace_bytes(lib):
    f = lib.dpvo_trajectory_ate_workspace_bytes
    assert f(40, 50) == 8 * 40 and f(50, 40) == 8 * 40 and f(65536, 65536) == 8 * 65536
    assert f(1, 1) > 0 and f(0, 0) > 0


def test_cpu_tensors_are_rejected_loudly():
    import torch

    import dpvo_amd
    from dpvo_amd import evaluation

    ext = dpvo_amd.load_extension("cuda_ba")
    assert hasattr(ext, "trajectory_ate")
    traj = torch.zeros(5, 7)
    ts = torch.arange(5, dtype=torch.float64)
    ref = torch.zeros(5, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluation.ate(traj, ts, ref, ts)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.trajectory_ate(ref, ts, ref, ts, 0.01, True)
    assert dpvo_amd.ate is evaluation.ate and dpvo_amd.ATEResult is evaluation.ATEResult
    assert dpvo_amd.read_tum is evaluation.read_tum and dpvo_amd.write_tum is evaluation.write_tum
