"""CPU: the tracker's entry points of the C ABI (dpvo_frame_sample,
dpvo_probe_median, dpvo_update_targets, dpvo_map_points) validate their
arguments before any launch -- no GPU needed -- and the public names exist."""
import ctypes

import pytest

INVALID, UNSUPPORTED = 1, 3
ONE = ctypes.c_void_p(1)  # a non-null pointer that is never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.dpvo_frame_sample.argtypes = [vp] * 6 + [i, vp, vp] + [i] * 12 + [vp, vp]
    lib.dpvo_probe_median.argtypes = [vp, i, i, vp, vp]
    lib.dpvo_update_targets.argtypes = [vp, vp, vp, i, vp, vp, i, i, vp, i, vp]
    lib.dpvo_map_points.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp, i, vp]
    return lib


def test_exports_exist(lib):
    for name in ("dpvo_frame_sample", "dpvo_probe_median", "dpvo_update_targets",
                 "dpvo_map_points"):
        assert hasattr(lib, name), name


def _frame_sample(lib, ptrs=None, dtype=0, h=6, w=9, H=24, W=36, C=128, DIM=384, M=5, P=3, res=4,
                  pmem=3, N=9, n=2, n_dev=None):
    p = [ONE] * 8 if ptrs is None else ptrs
    return lib.dpvo_frame_sample(p[0], p[1], p[2], p[3], p[4], p[5], dtype, p[6], p[7], h, w, H, W,
                                 C, DIM, M, P, res, pmem, N, n, n_dev, None)


def test_frame_sample_validation(lib):
    for k in range(8):
        ptrs = [ONE] * 8
        ptrs[k] = None
        assert _frame_sample(lib, ptrs) == INVALID, k
    assert _frame_sample(lib, P=2) == INVALID
    assert _frame_sample(lib, P=4) == INVALID
    assert _frame_sample(lib, P=0) == INVALID
    assert _frame_sample(lib, P=7) == INVALID  # wider than the 6-row map
    for name in ("h", "w", "H", "W", "C", "DIM", "M", "res", "pmem", "N"):
        assert _frame_sample(lib, **{name: 0}) == INVALID, name
        assert _frame_sample(lib, **{name: -1}) == INVALID, name
    assert _frame_sample(lib, n=-1) == INVALID
    assert _frame_sample(lib, n=9) == INVALID
    assert _frame_sample(lib, dtype=2) == UNSUPPORTED  # fp64 rings
    assert _frame_sample(lib, h=1 << 12, w=1 << 12) == UNSUPPORTED  # 2^31 map elements


def test_probe_median_validation(lib):
    assert lib.dpvo_probe_median(None, 0, 8, ONE, None) == INVALID
    assert lib.dpvo_probe_median(ONE, 0, 8, None, None) == INVALID
    assert lib.dpvo_probe_median(ONE, 0, 0, ONE, None) == INVALID
    assert lib.dpvo_probe_median(ONE, 0, -3, ONE, None) == INVALID
    assert lib.dpvo_probe_median(ONE, 2, 8, ONE, None) == INVALID
    assert lib.dpvo_probe_median(ONE, 0, 1025, ONE, None) == UNSUPPORTED
    assert lib.dpvo_probe_median(ONE, 1, 1 << 20, ONE, None) == UNSUPPORTED


def _update_targets(lib, ptrs=None, dtype=0, P=3, E=4, E_dev=None, cap=8):
    p = [ONE] * 5 if ptrs is None else ptrs
    return lib.dpvo_update_targets(p[0], p[1], p[2], dtype, p[3], p[4], P, E, E_dev, cap, None)


def test_update_targets_validation(lib):
    for k in range(5):
        ptrs = [ONE] * 5
        ptrs[k] = None
        assert _update_targets(lib, ptrs) == INVALID, k
    assert _update_targets(lib, P=2) == INVALID
    assert _update_targets(lib, P=0) == INVALID
    assert _update_targets(lib, E=-1) == INVALID
    assert _update_targets(lib, E=9) == INVALID  # more edges than rows
    assert _update_targets(lib, cap=-1) == INVALID
    assert _update_targets(lib, dtype=2) == INVALID
    # E == 0 is a no-op without a launch, whatever the pointers
    assert _update_targets(lib, E=0) == 0
    assert _update_targets(lib, [None] * 5, E=0) == 0


def _map_points(lib, ptrs=None, N=8, P=3, m=5, m_dev=None, cap=40):
    p = [ONE] * 5 if ptrs is None else ptrs
    return lib.dpvo_map_points(p[0], p[1], p[2], p[3], p[4], N, P, m, m_dev, cap, None)


def test_map_points_validation(lib):
    for k in range(5):
        ptrs = [ONE] * 5
        ptrs[k] = None
        assert _map_points(lib, ptrs) == INVALID, k
    assert _map_points(lib, P=2) == INVALID
    assert _map_points(lib, N=0) == INVALID
    assert _map_points(lib, m=-1) == INVALID
    assert _map_points(lib, m=41) == INVALID
    assert _map_points(lib, cap=-1) == INVALID
    assert _map_points(lib, m=0) == 0
    assert _map_points(lib, [None] * 5, m=0) == 0


def test_default_config_is_the_reference_table():
    import dpvo_amd

    cfg = dpvo_amd.default_config()
    assert vars(cfg) == dict(
        BUFFER_SIZE=4096, CENTROID_SEL_STRAT="RANDOM", PATCHES_PER_FRAME=80, REMOVAL_WINDOW=20,
        OPTIMIZATION_WINDOW=12, PATCH_LIFETIME=12, KEYFRAME_INDEX=4, KEYFRAME_THRESH=12.5,
        MOTION_MODEL="DAMPED_LINEAR", MOTION_DAMPING=0.5, MIXED_PRECISION=True,
        LOOP_CLOSURE=False, BACKEND_THRESH=64.0, MAX_EDGE_AGE=1000, GLOBAL_OPT_FREQ=15,
        CLASSIC_LOOP_CLOSURE=False, LOOP_CLOSE_WINDOW_SIZE=3, LOOP_RETR_THRESH=0.04,
        MAX_EDGES=10000)
    assert dpvo_amd.default_config() is not cfg  # a fresh namespace per call


def test_public_names_import():
    import dpvo_amd
    from dpvo_amd import DPVO, VONet, default_config, tracker  # noqa: F401

    assert callable(DPVO) and callable(VONet)
    for name in ("frame_sample", "probe_median", "update_targets", "map_points"):
        assert callable(getattr(tracker, name))
        assert hasattr(dpvo_amd.load_extension("cuda_ba"), name)


def test_vonet_loads_a_checkpoint_with_module_prefix_and_lmbda():
    import torch

    from dpvo_amd import VONet

    src = VONet(dtype=torch.float32)
    sd = {"module." + k: v.clone() + 1.0 for k, v in src.state_dict().items()}
    sd["module.update.lmbda"] = torch.zeros(1)
    dst = VONet(dtype=torch.float32)
    assert dst.load_checkpoint(sd) is dst
    for (k, a), b in zip(src.state_dict().items(), dst.state_dict().values()):
        assert torch.equal(a + 1.0, b), k
    assert (dst.DIM, dst.RES, dst.P) == (384, 4, 3)
    with pytest.raises(RuntimeError):
        dst.load_checkpoint({"module.update.extra": torch.zeros(1), **sd})


def test_cpu_tensors_are_rejected_loudly():
    import torch

    from dpvo_amd import tracker

    with pytest.raises(RuntimeError, match="GPU"):
        tracker.probe_median(torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        tracker.update_targets(torch.zeros(1, 4, 2, 3, 3), torch.zeros(1, 4, 2), torch.zeros(1, 4, 2),
                               torch.zeros(1, 8, 2), torch.zeros(1, 8, 2), 4)
    with pytest.raises(RuntimeError, match="GPU"):
        tracker.map_points(torch.zeros(2, 7), torch.zeros(4, 3, 3, 3), torch.zeros(2, 4),
                           torch.zeros(4, dtype=torch.long), torch.zeros(4, 3), 4)


def test_classic_loop_closure_is_the_callers_hook():
    import dpvo_amd

    cfg = dpvo_amd.default_config()
    cfg.CLASSIC_LOOP_CLOSURE = True
    with pytest.raises(NotImplementedError, match="close_loop"):
        dpvo_amd.DPVO(cfg, object(), device="cpu")
