"""GPU: the four kernels of csrc/tracker.hip against tests/tracker_ref.py.

frame_sample and update_targets copy or add once in fp32: bit-exact.
probe_median: within one fp32 ulp of torch.quantile on the CPU.  map_points:
|got - ref| <= 1e-5 max(1, |ref|) per point against the fp64 restatement (the
fp32 bar of reproject, 2e-4 px, carried to unit-scale points); the kernel
computes in fp64 and rounds once, so the worst case is one fp32 rounding of the
point (about 6e-8 relative)."""
import numpy as np
import pytest
import torch

import tracker_ref as R

pytestmark = pytest.mark.gpu


def _bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bit_equal(got, ref, what=""):
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), what
    np.testing.assert_array_equal(_bits(got), _bits(ref), what)


# ---- frame_sample ------------------------------------------------------------------
H_, W_, M_, P_, PMEM, NBUF, C_, DIM_ = 6, 9, 5, 3, 3, 9, 128, 384
CENTRES = [[1, 1], [W_ - 2, 1], [1, H_ - 2], [W_ - 2, H_ - 2], [4, 3]]


@pytest.fixture(scope="module")
def frame():
    """fmap, imap, the byte image (every value 0..255 occurs) and the centres."""
    g = torch.Generator().manual_seed(7)
    fmap = torch.randn(C_, H_, W_, generator=g)
    imap = torch.randn(DIM_, H_, W_, generator=g)
    count = 3 * 4 * H_ * 4 * W_
    byte = (torch.arange(count) * 37 % 256).to(torch.uint8).view(3, 4 * H_, 4 * W_)
    assert byte.unique().numel() == 256
    return fmap, imap, byte, torch.tensor(CENTRES, dtype=torch.float32)


def _run_frame_sample(gpu, fmap, imap, byte, coords, n, ring_dtype, n_as_tensor, M=M_):
    from dpvo_amd import tracker

    # normalised on the CPU: the values for which the chain is p - 1 on 31 bytes
    image = R.normalise(byte).to(gpu)
    gring = torch.full((PMEM, M, C_, P_, P_), 7.5, dtype=ring_dtype, device=gpu)
    iring = torch.full((PMEM, M, DIM_), -3.25, dtype=ring_dtype, device=gpu)
    colors = torch.full((NBUF, M, 3), 0xAB, dtype=torch.uint8, device=gpu)
    n_arg = torch.tensor([n], dtype=torch.int32, device=gpu) if n_as_tensor else n
    patches = tracker.frame_sample(fmap.to(gpu), imap.to(gpu), image, coords.to(gpu), gring, iring,
                                   colors, n_arg)
    torch.cuda.synchronize()
    return image, gring, iring, colors, patches


@pytest.mark.parametrize("n_as_tensor", [False, True])
@pytest.mark.parametrize("ring_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n", [0, 2, 3, 7])
def test_frame_sample(gpu, frame, n, ring_dtype, n_as_tensor):
    fmap, imap, byte, coords = frame
    image, gring, iring, colors, patches = _run_frame_sample(gpu, fmap, imap, byte, coords, n,
                                                             ring_dtype, n_as_tensor)
    g, im, pt, clr = R.frame_sample(fmap, imap, R.normalise(byte), coords, P_, ring_dtype)
    slot = n % PMEM
    assert_bit_equal(gring[slot].cpu(), g, "gmap ring row")
    assert_bit_equal(iring[slot].cpu(), im, "imap ring row")
    assert_bit_equal(patches.cpu(), pt, "patch grid")
    assert_bit_equal(colors[n].cpu(), clr, "colours")
    for s in range(PMEM):
        if s != slot:
            assert (gring[s] == 7.5).all() and (iring[s] == -3.25).all(), s
    rest = torch.ones(NBUF, dtype=torch.bool)
    rest[n] = False
    assert (colors.cpu()[rest] == 0xAB).all()


def test_frame_sample_colours_over_every_byte_value(gpu, frame):
    """Every legal centre of the map (28 of them, 84 colour samples a call) over
    four images whose sampled pixels run through all 256 byte values: the 31
    values on which the reference's chain is not the identity are among them."""
    fmap, imap, _, _ = frame
    ys, xs = torch.meshgrid(torch.arange(1, H_ - 1), torch.arange(1, W_ - 1), indexing="ij")
    coords = torch.stack([xs.reshape(-1), ys.reshape(-1)], -1).float()
    M = coords.shape[0]
    seen = set()
    for k in range(4):
        byte = torch.zeros(3, 4 * H_, 4 * W_, dtype=torch.uint8)
        vals = ((torch.arange(3 * M) + 84 * k) % 256).to(torch.uint8).view(3, M)
        byte[:, 4 * coords[:, 1].long() + 2, 4 * coords[:, 0].long() + 2] = vals
        _, _, _, colors, _ = _run_frame_sample(gpu, fmap, imap, byte, coords, 1, torch.float32,
                                               False, M=M)
        ref = R.color_chain(vals).T[:, [2, 1, 0]].contiguous()
        assert_bit_equal(colors[1].cpu(), ref, f"image {k}")
        seen.update(vals.reshape(-1).tolist())
    assert len(seen) == 256


def test_frame_sample_rejects_bad_arguments(gpu, frame):
    from dpvo_amd import tracker

    fmap, imap, byte, coords = (t.to(gpu) for t in frame)
    image = R.normalise(byte)
    gring = torch.zeros(PMEM, M_, C_, P_, P_, device=gpu)
    iring = torch.zeros(PMEM, M_, DIM_, device=gpu)
    colors = torch.zeros(NBUF, M_, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError):
        tracker.frame_sample(fmap, imap, image, coords, gring, iring, colors, NBUF)
    with pytest.raises(RuntimeError):
        tracker.frame_sample(fmap, imap, image, coords, gring, iring.half(), colors, 0)
    with pytest.raises(RuntimeError):
        tracker.frame_sample(fmap, imap, image, coords, gring, iring, colors.int(), 0)


# ---- probe_median ------------------------------------------------------------------
def _ulp_apart(a, b):
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 30
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))  # both >= 0: norms


@pytest.fixture(scope="module")
def deltas():
    g = torch.Generator().manual_seed(3)
    return {M: 3.0 * torch.randn(M, 2, generator=g) for M in (1, 2, 7, 8, 80, 96, 1024)}


@pytest.mark.parametrize("M", [1, 2, 7, 8, 80, 96, 1024])
def test_probe_median(gpu, deltas, M):
    from dpvo_amd import tracker

    d = deltas[M]
    got = tracker.probe_median(d.to(gpu))
    assert got.dtype == torch.float32 and got.dim() == 0
    ref = R.probe_median(d)
    print(f"M={M}: got {float(got):.9g} ref {float(ref):.9g}")
    assert _ulp_apart(got.item(), ref.item()) <= 1
    if M == 1:
        assert _ulp_apart(got.item(), d.norm().item()) <= 1
    # the shapes the tracker passes: [1, M, 2]
    assert _ulp_apart(tracker.probe_median(d.to(gpu)[None]).item(), ref.item()) <= 1


@pytest.mark.parametrize("M", [8, 80, 81])
def test_probe_median_ties_nan_half(gpu, deltas, M):
    from dpvo_amd import tracker

    g = torch.Generator().manual_seed(M)
    # ties: only three distinct rows
    pool = torch.tensor([[3.0, 4.0], [0.6, 0.8], [1.5, 2.0]])
    d = pool[torch.randint(0, 3, (M,), generator=g)]
    assert _ulp_apart(tracker.probe_median(d.to(gpu)).item(), R.probe_median(d).item()) <= 1
    d = torch.zeros(M, 2)
    assert tracker.probe_median(d.to(gpu)).item() == 0.0
    # one NaN anywhere gives NaN, as torch.quantile does
    d = 3.0 * torch.randn(M, 2, generator=g)
    d[M // 3, 1] = float("nan")
    assert torch.isnan(R.probe_median(d)) and torch.isnan(tracker.probe_median(d.to(gpu)))
    # fp16 input is widened first
    d = (3.0 * torch.randn(M, 2, generator=g)).half()
    assert _ulp_apart(tracker.probe_median(d.to(gpu)).item(), R.probe_median(d).item()) <= 1


def test_probe_median_above_one_workgroup_is_unsupported(gpu):
    from dpvo_amd import tracker

    with pytest.raises(RuntimeError, match="status 3"):
        tracker.probe_median(torch.zeros(1025, 2, device=gpu))


# ---- update_targets ----------------------------------------------------------------
@pytest.fixture(scope="module")
def edges300():
    g = torch.Generator().manual_seed(5)
    coords = 100.0 * torch.rand(1, 300, 2, 3, 3, generator=g)
    delta = 4.0 * torch.randn(1, 300, 2, generator=g)
    w = torch.rand(1, 300, 2, generator=g)
    return coords, delta, w


@pytest.mark.parametrize("E_as_tensor", [False, True])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("E", [0, 1, 65, 257])
def test_update_targets(gpu, edges300, E, half, E_as_tensor):
    from dpvo_amd import tracker

    coords, delta, w = edges300
    if half:
        delta, w = delta.half(), w.half()
    target = torch.full((1, 300, 2), 11.0, device=gpu)
    weight = torch.full((1, 300, 2), 13.0, device=gpu)
    E_arg = torch.tensor([E], dtype=torch.int32, device=gpu) if E_as_tensor else E
    # the tracker passes the E-row slices of coords / delta / w and the whole pg buffers
    rows = 300 if E_as_tensor else E
    tracker.update_targets(coords[:, :rows].to(gpu), delta[:, :rows].to(gpu), w[:, :rows].to(gpu),
                           target, weight, E_arg)
    torch.cuda.synchronize()
    rt, rw = R.update_targets(coords[:, :E], delta[:, :E], w[:, :E])
    assert_bit_equal(target[:, :E].cpu(), rt, "target")
    assert_bit_equal(weight[:, :E].cpu(), rw, "weight")
    assert (target[:, E:] == 11.0).all() and (weight[:, E:] == 13.0).all()


# ---- map_points --------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(9)
    N, M, P = 8, 5, 3
    q = rng.normal(size=(N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.concatenate([rng.normal(size=(N, 3)), q], 1).astype(np.float32)
    patches = np.empty((N * M, 3, P, P), np.float32)
    patches[:, 0] = rng.uniform(0, 160, size=(N * M, P, P))
    patches[:, 1] = rng.uniform(0, 120, size=(N * M, P, P))
    patches[:, 2] = rng.uniform(0.1, 2.0, size=(N * M, P, P))
    intr = np.tile(np.float32([80.0, 85.0, 80.0, 60.0]), (N, 1)) + rng.uniform(0, 1, (N, 4)).astype(np.float32)
    ix = np.repeat(np.arange(N), M).astype(np.int64)
    rng.shuffle(ix)  # any patch -> frame map, not only the tracker's
    return poses, patches, intr, ix


@pytest.mark.parametrize("m_as_tensor", [False, True])
@pytest.mark.parametrize("m", [0, 1, 5, 23])
def test_map_points(gpu, scene, m, m_as_tensor):
    from dpvo_amd import tracker

    poses, patches, intr, ix = scene
    points = torch.full((40, 3), 17.0, device=gpu)
    m_arg = torch.tensor([m], dtype=torch.int32, device=gpu) if m_as_tensor else m
    tracker.map_points(*(torch.from_numpy(a).to(gpu) for a in scene), points, m_arg)
    torch.cuda.synchronize()
    got = points.cpu().numpy().astype(np.float64)
    ref = R.map_points(poses, patches, intr, ix, m)
    assert (got[m:] == 17.0).all()
    if m:
        err = np.linalg.norm(got[:m] - ref, axis=1)
        lim = 1e-5 * np.maximum(1.0, np.linalg.norm(ref, axis=1))
        print(f"m={m}: worst err / max(1, |ref|) = {float((err / (lim / 1e-5)).max()):.3g}")
        assert (err <= lim).all(), float((err / lim).max())


def test_map_points_zero_depth_divides(gpu, scene):
    from dpvo_amd import tracker

    poses, patches, intr, ix = (torch.from_numpy(a).to(gpu) for a in scene)
    patches = patches.clone()
    patches[2, 2] = 0.0
    points = torch.zeros(40, 3, device=gpu)
    tracker.map_points(poses, patches, intr, ix, points, 5)
    torch.cuda.synchronize()
    assert not torch.isfinite(points[2]).any()
    assert torch.isfinite(points[:2]).all() and torch.isfinite(points[3:5]).all()
