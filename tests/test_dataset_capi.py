"""CPU: host-side validation of the dataset entries of the C ABI
(dpvo_frame_flow_distance, dpvo_frame_graph_*, dpvo_rgbd_augment,
dpvo_normalize_depth), before any launch -- no GPU needed."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED = 0, 1, 3
ONE = ctypes.c_void_p(16)   # non-null, aligned, never dereferenced on the host
ODD = ctypes.c_void_p(18)   # not 4-byte aligned


class AugmentParams(ctypes.Structure):
    _fields_ = [("do_color", ctypes.c_int), ("order", ctypes.c_int * 4),
                ("brightness", ctypes.c_float), ("contrast", ctypes.c_float),
                ("saturation", ctypes.c_float), ("hue", ctypes.c_float), ("gray", ctypes.c_int),
                ("invert", ctypes.c_int), ("scale", ctypes.c_double), ("swap_rb", ctypes.c_int)]


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.dpvo_frame_flow_distance.argtypes = [vp, vp, vp, i, i, i, vp, vp]
    lib.dpvo_frame_graph_count.argtypes = [vp, i, f, f, vp, vp]
    lib.dpvo_frame_graph_fill.argtypes = [vp, i, f, f, vp, vp, vp, i, vp]
    lib.dpvo_rgbd_augment_workspace_bytes.restype = ctypes.c_size_t
    lib.dpvo_rgbd_augment.argtypes = [vp, vp, vp, i, i, i, i, i, ctypes.POINTER(AugmentParams), vp,
                                      vp, vp, vp, ctypes.c_size_t, vp]
    lib.dpvo_normalize_depth.argtypes = [vp, i, vp, i, vp, vp, vp, vp]
    return lib


def _dist(lib, poses=ONE, disps=ONE, intr=ONE, N=5, h=6, w=8, D=ONE):
    return lib.dpvo_frame_flow_distance(poses, disps, intr, N, h, w, D, None)


def test_distance_pointers(lib):
    for k in ("poses", "disps", "intr", "D"):
        assert _dist(lib, **{k: None}) == INVALID
        assert _dist(lib, **{k: ODD}) == INVALID


def test_distance_sizes(lib):
    assert _dist(lib, N=0) == INVALID
    assert _dist(lib, N=-3) == INVALID
    assert _dist(lib, h=0) == INVALID
    assert _dist(lib, w=-1) == INVALID
    assert _dist(lib, N=8193) == UNSUPPORTED
    assert _dist(lib, h=257, w=256) == UNSUPPORTED
    assert _dist(lib, h=65536, w=65536) == UNSUPPORTED   # h w past int
    # invalid wins over unsupported
    assert _dist(lib, N=8193, h=0) == INVALID
    assert _dist(lib, N=8193, D=None) == INVALID
    assert _dist(lib, h=257, w=256, poses=ODD) == INVALID


def test_graph_arguments(lib):
    cnt = lambda **k: lib.dpvo_frame_graph_count(k.get("D", ONE), k.get("N", 5), k.get("f", 16.0),  # noqa: E731
                                                 k.get("m", 256.0), k.get("rowptr", ONE), None)
    fill = lambda **k: lib.dpvo_frame_graph_fill(k.get("D", ONE), k.get("N", 5), k.get("f", 16.0),  # noqa: E731
                                                 k.get("m", 256.0), k.get("rowptr", ONE),
                                                 k.get("col", ONE), k.get("dist", ONE),
                                                 k.get("nnz", 3), None)
    for fn in (cnt, fill):
        assert fn(D=None) == INVALID
        assert fn(D=ODD) == INVALID
        assert fn(rowptr=None) == INVALID
        assert fn(N=0) == INVALID
        assert fn(f=0.0) == INVALID
        assert fn(f=float("inf")) == INVALID
        assert fn(m=float("nan")) == INVALID
        assert fn(N=8193) == UNSUPPORTED
        assert fn(N=8193, D=None) == INVALID
    assert fill(col=None) == INVALID
    assert fill(dist=ODD) == INVALID
    assert fill(nnz=-1) == INVALID
    assert fill(nnz=0, col=None, dist=None) == OK   # nothing to write, nothing launched


def _params(**kw):
    p = AugmentParams(1, (ctypes.c_int * 4)(0, 1, 2, 3), 1.1, 0.9, 1.2, 0.05, 0, 0, 1.0, 0)
    for k, v in kw.items():
        setattr(p, k, (ctypes.c_int * 4)(*v) if k == "order" else v)
    return p


def _aug(lib, N=2, H=20, W=28, ch=16, cw=24, ws_bytes=None, null=None, odd=None, **kw):
    ptr = {k: ONE for k in ("images", "disps", "intr", "images_out", "disps_out", "intr_out", "ws")}
    if null:
        ptr[null] = None
    if odd:
        ptr[odd] = ODD
    p = _params(**kw)
    if ws_bytes is None:
        ws_bytes = max(lib.dpvo_rgbd_augment_workspace_bytes(N, H, W), 2048)
    return lib.dpvo_rgbd_augment(ptr["images"], ptr["disps"], ptr["intr"], N, H, W, ch, cw,
                                 ctypes.byref(p), ptr["images_out"], ptr["disps_out"],
                                 ptr["intr_out"], ptr["ws"], ws_bytes, None)


def test_augment_pointers_and_sizes(lib):
    for k in ("images", "disps", "intr", "images_out", "disps_out", "intr_out", "ws"):
        assert _aug(lib, null=k) == INVALID
        assert _aug(lib, odd=k) == INVALID
    assert lib.dpvo_rgbd_augment(ONE, ONE, ONE, 2, 20, 28, 16, 24, None, ONE, ONE, ONE, ONE, 1 << 20,
                                 None) == INVALID
    for k in ("N", "H", "W", "ch", "cw"):
        assert _aug(lib, **{k: 0}) == INVALID
        assert _aug(lib, **{k: -2}) == INVALID
    assert _aug(lib, H=20000, ch=16) == UNSUPPORTED
    assert _aug(lib, N=1 << 20, H=480, W=640, ws_bytes=1 << 40) == UNSUPPORTED
    assert _aug(lib, H=20000, ch=0) == INVALID            # invalid wins
    assert _aug(lib, H=20000, order=(0, 1, 2, 2)) == INVALID


def test_augment_crop_must_fit(lib):
    # a resized frame: the crop may be at most int(scale * size) - 1
    s = 1.37
    ht1, wd1 = int(s * 20), int(s * 28)
    assert _aug(lib, scale=s, ch=ht1, cw=24) == INVALID
    assert _aug(lib, scale=s, ch=16, cw=wd1) == INVALID
    assert _aug(lib, scale=s, ch=ht1 + 5, cw=24) == INVALID
    # scale 1 resamples nothing: the crop may be the frame, not more
    assert _aug(lib, scale=1.0, ch=21, cw=24) == INVALID
    assert _aug(lib, scale=1.0, ch=16, cw=29) == INVALID


@pytest.mark.parametrize("order", [(0, 1, 2, 2), (0, 0, 0, 0), (1, 2, 3, 4), (-1, 0, 1, 2),
                                   (3, 2, 1, 3)])
def test_augment_order_is_a_permutation(lib, order):
    assert _aug(lib, order=order) == INVALID


@pytest.mark.parametrize("field", ["brightness", "contrast", "saturation", "hue", "scale"])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_augment_parameters_are_finite(lib, field, bad):
    assert _aug(lib, **{field: bad}) == INVALID


def test_augment_flags_and_scale(lib):
    for k in ("do_color", "gray", "invert", "swap_rb"):
        assert _aug(lib, **{k: 2}) == INVALID
        assert _aug(lib, **{k: -1}) == INVALID
    assert _aug(lib, scale=0.0) == INVALID
    assert _aug(lib, scale=-1.0) == INVALID
    assert _aug(lib, brightness=-0.5) == INVALID


def test_augment_workspace(lib):
    WORKSPACE = 4
    assert lib.dpvo_rgbd_augment_workspace_bytes(2, 20, 28) == 2048 + 4 * 3 * 2 * 20 * 28
    assert _aug(lib, ws_bytes=100) == WORKSPACE
    assert _aug(lib, scale=1.37, ws_bytes=2048) == WORKSPACE   # colour, then resampling: scratch


def test_normalize_arguments(lib):
    nd = lambda **k: lib.dpvo_normalize_depth(k.get("disps", ONE), k.get("n", 768), k.get("poses", ONE),  # noqa: E731
                                              k.get("np", 2), k.get("dout", ONE), k.get("pout", ONE),
                                              k.get("s", ONE), None)
    for k in ("disps", "poses", "dout", "pout", "s"):
        assert nd(**{k: None}) == INVALID
        assert nd(**{k: ODD}) == INVALID
    assert nd(n=0) == INVALID
    assert nd(np=0) == INVALID
    assert nd(n=(1 << 30) + 1) == UNSUPPORTED
    assert nd(n=(1 << 30) + 1, poses=None) == INVALID


def test_cpu_tensors_are_rejected_loudly():
    import torch

    import dpvo_amd
    from dpvo_amd import data_readers as dr

    ext = dpvo_amd.load_extension("cuda_ba")
    for name in ("frame_flow_distance", "frame_graph", "rgbd_augment", "normalize_depth"):
        assert hasattr(ext, name)
    with pytest.raises(RuntimeError, match="GPU"):
        dr.frame_distance_matrix(torch.zeros(3, 7), torch.ones(3, 4, 4), torch.ones(3, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        dr.RGBDAugmentor((4, 4))(torch.zeros(1, 3, 8, 8), torch.zeros(1, 7), torch.ones(1, 8, 8),
                                 torch.ones(1, 4), params=dr.AugmentParams())
    with pytest.raises(RuntimeError, match="GPU"):
        dr.normalize_depth(torch.ones(8), torch.zeros(1, 7))
    assert dpvo_amd.TartanAir is dr.TartanAir and dpvo_amd.build_frame_graph is dr.build_frame_graph
    assert dpvo_amd.RGBDAugmentor is dr.RGBDAugmentor and dpvo_amd.FrameGraph is dr.FrameGraph
