"""GPU: the frame front-end and the trajectory read-out (csrc/frontend.hip,
dpvo_amd/frontend.py) against tests/frontend_ref.py and torch.median.

Tolerance of every pose comparison (derived): the kernels compute in fp64 from
the same fp32 inputs as the restatement, so the only rounding above ~1e-12 is
the final store to fp32.  Per component |got - ref| <= 2^-21 max(1, |ref|),
four fp32 ulps at the component's scale; quaternions compared up to a common
sign.  Medians, copies, timestamps and intrinsics are bit-exact."""
import numpy as np
import pytest
import torch

import frontend_ref as F
import se3_restatement as R

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -21


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bit_equal(got, ref, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(ref), what)


def assert_pose_close(got, ref, what=""):
    """rows [..., 7]; NaN rows of ref must be NaN rows of got."""
    got = np.asarray(got, np.float64).reshape(-1, 7)
    ref = np.asarray(ref, np.float64).reshape(-1, 7).copy()
    bad = np.isnan(ref).any(1)
    assert np.isnan(got[bad]).all(), what
    assert not np.isnan(got[~bad]).any(), what
    got, ref = got[~bad], ref[~bad]
    flip = (got[:, 3:] * ref[:, 3:]).sum(1) < 0
    ref[flip, 3:] *= -1
    err = np.abs(got - ref)
    lim = TOL * np.maximum(1.0, np.abs(ref))
    assert (err <= lim).all(), (what, float((err / lim).max()))
    np.testing.assert_allclose(np.linalg.norm(got[:, 3:], axis=1), 1.0, atol=TOL, err_msg=what)


def _pose(rng, rot=0.3, trans=1.0):
    xi = np.concatenate([trans * rng.normal(size=3), rot * rng.normal(size=3)])
    return R.to_data(R.Exp(torch.as_tensor(xi))).numpy()


def _compose(xi, P):
    """Exp(xi) * P as data [7] (fp64)."""
    return R.to_data(R.Exp(torch.as_tensor(np.asarray(xi, np.float64))) @
                     R.from_data(torch.as_tensor(P))).numpy()


def _state(rng, N, M, P):
    poses = np.stack([_pose(rng) for _ in range(N)]).astype(np.float32)
    patches = rng.uniform(0.1, 5.0, size=(N * M, 3, P, P)).astype(np.float32)
    intr = rng.uniform(50, 400, size=(N, 4)).astype(np.float32)
    tstamps = rng.integers(0, 1000, size=N).astype(np.int64)
    return poses, patches, intr, tstamps


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


# ---- median -----------------------------------------------------------------------

def _values(kind, rng, count):
    if kind == "positive":
        return rng.uniform(0.01, 5.0, count).astype(np.float32)
    if kind == "mixed":
        v = rng.normal(size=count).astype(np.float32)
        v[v == 0] = 1.0  # no +-0: torch.median's choice between them is not specified
        return v
    if kind == "equal":
        return np.full(count, 0.7, np.float32)
    if kind == "two":
        v = np.where(np.arange(count) < count // 2, 0.25, 0.75).astype(np.float32)
        return rng.permutation(v)
    if kind == "denormal":
        u = rng.integers(1, 1 << 23, count).astype(np.uint32)
        u |= (rng.integers(0, 2, count).astype(np.uint32) << 31)
        return u.view(np.float32)
    if kind == "lowbyte":
        return (np.uint32(0x3F800000) | rng.integers(0, 256, count).astype(np.uint32)).view(
            np.float32)
    if kind == "nan":
        v = rng.uniform(0.01, 5.0, count).astype(np.float32)
        v[rng.integers(0, count)] = np.nan
        return v
    raise ValueError(kind)


SHAPES = [(3, 1, 1), (3, 2, 3), (3, 7, 3), (2, 5, 3), (1, 5, 3), (9, 96, 3)]
KINDS = ["positive", "mixed", "equal", "two", "denormal", "lowbyte", "nan"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,M,P", SHAPES)
def test_median_depth_is_torch_median(gpu, n, M, P, kind):
    from dpvo_amd import frontend

    rng = np.random.default_rng(1000 * n + 10 * M + P + 7 * KINDS.index(kind))
    N = n + 2
    poses, patches, intr, tstamps = _state(rng, N, M, P)
    f0 = max(n - 3, 0)
    # rows outside the window would change the answer if they were read
    patches[:f0 * M, 2] = 1e9
    patches[n * M:, 2] = -1e9
    count = (n - f0) * M * P * P
    patches[f0 * M:n * M, 2] = _values(kind, rng, count).reshape(n - f0, M, P, P).reshape(-1, P, P)
    new = rng.uniform(0.1, 5.0, size=(1, M, 3, P, P)).astype(np.float32)
    ni = np.array([320.0, 330.0, 160.0, 120.0], np.float32)
    times = np.arange(16, dtype=np.float64)
    dP, dK, dI, dT, dtm, dnew, dni = _dev(gpu, poses, patches, intr, tstamps, times, new, ni)
    frontend.init_frame(dP, dK, dI, dT, dtm, dnew, dni, n, 5, M, median=True)
    got = dK.cpu().numpy()
    s = torch.median(torch.from_numpy(patches[f0 * M:n * M, 2]))
    row = got[n * M:(n + 1) * M]
    if kind == "nan":
        assert torch.isnan(s) and np.isnan(row[:, 2]).all()
    else:
        assert_bit_equal(row[:, 2], np.full((M, P, P), s.item(), np.float32), "depth = median")
    assert_bit_equal(row[:, :2], new[0, :, :2], "channels 0, 1")
    assert_bit_equal(got[:n * M], patches[:n * M], "rows before n")
    assert_bit_equal(got[(n + 1) * M:], patches[(n + 1) * M:], "rows after n")


@pytest.mark.parametrize("n", [0, 3])
def test_median_off_or_first_frame_keeps_depth(gpu, n):
    from dpvo_amd import frontend

    rng = np.random.default_rng(n)
    N, M, P = 6, 7, 3
    poses, patches, intr, tstamps = _state(rng, N, M, P)
    new = rng.uniform(0.1, 5.0, size=(M, 3, P, P)).astype(np.float32)
    ni = np.array([320.0, 330.0, 160.0, 120.0], np.float32)
    dP, dK, dI, dT, dtm, dnew, dni = _dev(gpu, poses, patches, intr, tstamps,
                                          np.arange(16, dtype=np.float64), new, ni)
    # n = 0 keeps it even with median on (nothing to take a median of)
    frontend.init_frame(dP, dK, dI, dT, dtm, dnew, dni, n, 5, M, median=(n == 0))
    got = dK.cpu().numpy()
    assert_bit_equal(got[n * M:(n + 1) * M], new)
    assert_bit_equal(np.delete(got, np.s_[n * M:(n + 1) * M], 0),
                     np.delete(patches, np.s_[n * M:(n + 1) * M], 0))


# ---- motion model -----------------------------------------------------------------

def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _pair(case, rng):
    """(P1, P2) fp32: P1 = Exp(xi) P2 in fp64, rounded."""
    P2 = _pose(rng)
    xi = {
        "small": np.concatenate([0.05 * rng.normal(size=3), 0.02 * rng.normal(size=3)]),
        "equal": np.zeros(6),
        "rot2": np.concatenate([0.3 * rng.normal(size=3), 2.0 * _unit(rng)]),
        "tinyrot": np.concatenate([0.1 * _unit(rng), 5e-7 * _unit(rng)]),
        "trans1e-3": np.concatenate([1e-3 * _unit(rng), 0.02 * rng.normal(size=3)]),
        "trans1e2": np.concatenate([1e2 * _unit(rng), 0.02 * rng.normal(size=3)]),
    }[case]
    P1 = P2 if case == "equal" else _compose(xi, P2)
    return P1.astype(np.float32), P2.astype(np.float32)


@pytest.mark.parametrize("case", ["small", "equal", "rot2", "tinyrot", "trans1e-3", "trans1e2"])
def test_motion_model_matches_restatement(gpu, case):
    from dpvo_amd import frontend

    rng = np.random.default_rng(sum(map(ord, case)))
    N, M, P, n, counter = 6, 2, 3, 3, 9
    poses, patches, intr, tstamps = _state(rng, N, M, P)
    poses[n - 1], poses[n - 2] = _pair(case, rng)
    new = rng.uniform(0.1, 5.0, size=(M, 3, P, P)).astype(np.float32)
    ni = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
    for fac in (0.5, 1.0, 3.0, None):  # None: b == a, fac = 1
        times = np.zeros(16)
        times[counter - 2:counter + 1] = [4.0, 4.0, 5.0] if fac is None else [4.0, 5.0, 5.0 + fac]
        for damping in (0.0, 0.5, 1.0):
            for res in (4.0, 3.0):
                dP, dK, dI, dT, dtm, dnew, dni = _dev(gpu, poses, patches, intr, tstamps, times,
                                                      new, ni)
                frontend.init_frame(dP, dK, dI, dT, dtm, dnew, dni, n, counter, M,
                                    damping=damping, res=res)
                got = dP.cpu().numpy()
                what = f"{case} fac={fac} damping={damping}"
                assert F.time_factor(times, counter) == (1.0 if fac is None else fac)
                ref = F.motion_model(poses[n - 1], poses[n - 2], 1.0 if fac is None else fac,
                                     damping)
                assert_pose_close(got[n], ref, what)
                if case == "equal" or damping == 0.0:
                    assert_pose_close(got[n], F._data(F._mat(poses[n - 1])), what + " -> P1")
                assert_bit_equal(np.delete(got, n, 0), np.delete(poses, n, 0), what)
                gT, gI = dT.cpu().numpy(), dI.cpu().numpy()
                assert gT[n] == counter
                assert_bit_equal(gI[n], (torch.from_numpy(ni) / res).numpy(), "intrinsics / res")
                np.testing.assert_array_equal(np.delete(gT, n), np.delete(tstamps, n))
                assert_bit_equal(np.delete(gI, n, 0), np.delete(intr, n, 0))


@pytest.mark.parametrize("n", [0, 1])
def test_first_two_frames_keep_their_pose(gpu, n):
    from dpvo_amd import frontend

    rng = np.random.default_rng(n + 50)
    N, M, P = 5, 3, 3
    poses, patches, intr, tstamps = _state(rng, N, M, P)
    new = rng.uniform(0.1, 5.0, size=(M, 3, P, P)).astype(np.float32)
    ni = np.array([320.0, 330.0, 160.0, 120.0], np.float32)
    dP, dK, dI, dT, dtm, dnew, dni = _dev(gpu, poses, patches, intr, tstamps,
                                          np.arange(8, dtype=np.float64), new, ni)
    frontend.init_frame(dP, dK, dI, dT, dtm, dnew, dni, n, n, M)
    assert_bit_equal(dP.cpu().numpy(), poses)
    assert dT.cpu().numpy()[n] == n


def test_copy_model_copies_previous_pose(gpu):
    from dpvo_amd import frontend

    rng = np.random.default_rng(60)
    N, M, P, n = 5, 3, 3, 4
    poses, patches, intr, tstamps = _state(rng, N, M, P)
    poses[n - 1, 3:] *= 1.37  # not a unit quaternion: a copy must not normalise it
    new = rng.uniform(0.1, 5.0, size=(M, 3, P, P)).astype(np.float32)
    ni = np.array([320.0, 330.0, 160.0, 120.0], np.float32)
    dP, dK, dI, dT, dtm, dnew, dni = _dev(gpu, poses, patches, intr, tstamps,
                                          np.arange(8, dtype=np.float64), new, ni)
    frontend.init_frame(dP, dK, dI, dT, dtm, dnew, dni, n, 6, M, motion_model="CONSTANT")
    ref = poses.copy()
    ref[n] = poses[n - 1]
    assert_bit_equal(dP.cpu().numpy(), ref)


# ---- device scalars, graph replay -------------------------------------------------

def test_device_scalars_and_graph_replay(gpu):
    from dpvo_amd import frontend

    rng = np.random.default_rng(70)
    N, M, P = 10, 7, 3
    poses, patches, intr, tstamps = _state(rng, N, M, P)
    for f in range(1, N):  # a smooth track, so the motion model extrapolates something
        poses[f] = _compose(np.concatenate([0.05 * rng.normal(size=3), 0.02 * rng.normal(size=3)]),
                            poses[f - 1].astype(np.float64)).astype(np.float32)
    times = np.cumsum(rng.uniform(0.5, 1.5, 32))
    ni = np.array([320.0, 330.0, 160.0, 120.0], np.float32)
    new = rng.uniform(0.1, 5.0, size=(M, 3, P, P)).astype(np.float32)
    dP, dK, dI, dT, dtm, dnew, dni = _dev(gpu, poses, patches, intr, tstamps, times, new, ni)
    bufs = (dP, dK, dI, dT)
    n_dev = torch.tensor([3], dtype=torch.int32, device=gpu)
    c_dev = torch.tensor([11], dtype=torch.int32, device=gpu)

    def eager(n, counter):
        cl = [b.clone() for b in bufs]
        frontend.init_frame(*cl, dtm, dnew, dni, n, counter, M)
        return cl

    a, b = eager(3, 11), eager(3, 11)
    for x, y in zip(a, b):
        assert torch.equal(x, y)  # deterministic

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm on a side stream, on clones
        frontend.init_frame(*[t.clone() for t in bufs], dtm, dnew, dni, n_dev, c_dev, M)
    torch.cuda.current_stream().wait_stream(s)
    backup = [t.clone() for t in bufs]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        frontend.init_frame(dP, dK, dI, dT, dtm, dnew, dni, n_dev, c_dev, M)
    for t, bk in zip(bufs, backup):
        t.copy_(bk)
    for k in range(3):
        n, counter = 3 + k, 11 + 2 * k
        n_dev.fill_(n)
        c_dev.fill_(counter)
        dtm[counter] = float(times[counter - 1] + rng.uniform(0.5, 1.5))  # the caller's new time
        dnew.copy_(torch.from_numpy(rng.uniform(0.1, 5.0, size=(M, 3, P, P)).astype(np.float32)))
        ref = eager(n, counter)
        g.replay()
        torch.cuda.synchronize()
        for name, got, want in zip(("poses", "patches", "intrinsics", "tstamps"), bufs, ref):
            assert torch.equal(got, want), (k, name)
        assert_bit_equal(dP.cpu().numpy(), ref[0].cpu().numpy())


# ---- trajectory -------------------------------------------------------------------

def _delta(gpu, records, cap=None):
    cap = max(len(records), 1) if cap is None else cap
    log = np.zeros((cap, 7), np.float32)
    pairs = np.zeros((cap, 2), np.int64)
    for r, (t1, t0, dP) in enumerate(records):
        log[r], pairs[r] = dP, (t1, t0)
    dl, dp = _dev(gpu, log, pairs)
    return dl, dp, torch.tensor([len(records)], dtype=torch.int32, device=gpu)


def _check_trajectory(gpu, poses, tstamps, n, records, counter, n_as_tensor=False):
    from dpvo_amd import frontend

    dP, dT = _dev(gpu, poses, tstamps)
    delta = _delta(gpu, records)
    nn = torch.tensor([n], dtype=torch.int32, device=gpu) if n_as_tensor else n
    out = {}
    for inverse in (False, True):
        traj, root, info = frontend.trajectory(dP, dT, nn, delta, counter, inverse=inverse)
        rt, rr, ri = F.trajectory(poses, tstamps, n, records, counter, inverse=inverse)
        assert traj.shape == (counter, 7) and traj.dtype == torch.float32
        assert root.dtype == torch.int64 and info.dtype == torch.int32
        np.testing.assert_array_equal(root.cpu().numpy(), rr)
        np.testing.assert_array_equal(info.cpu().numpy(), ri)
        assert_pose_close(traj.cpu().numpy(), rt, f"inverse={inverse}")
        out[inverse] = traj.cpu().numpy()
    ok = ~np.isnan(out[False]).any(1)
    A = R.from_data(torch.from_numpy(out[True][ok]))
    B = R.from_data(torch.from_numpy(out[False][ok]))
    scale = np.maximum(1.0, np.linalg.norm(out[False][ok, :3], axis=1))[:, None, None]
    assert (np.abs((A @ B).numpy() - np.eye(4)) <= TOL * scale).all()
    return out


def _records_chain(rng, frames, step=0.05):
    return [(t, t - 1, _pose(rng, rot=0.03, trans=step).astype(np.float32)) for t in frames]


@pytest.mark.parametrize("counter", [1, 2])
def test_trajectory_smallest(gpu, counter):
    rng = np.random.default_rng(80 + counter)
    poses = np.stack([_pose(rng) for _ in range(4)]).astype(np.float32)
    tstamps = np.array([0, 7, 8, 9], np.int64)
    _check_trajectory(gpu, poses, tstamps, 1, _records_chain(rng, range(1, counter)), counter)


def test_trajectory_all_keyframes(gpu):
    rng = np.random.default_rng(83)
    poses = np.stack([_pose(rng) for _ in range(10)]).astype(np.float32)
    tstamps = np.arange(10, dtype=np.int64)
    out = _check_trajectory(gpu, poses, tstamps, 8, [], 8)
    assert not np.isnan(out[False]).any()


def test_trajectory_chain_depths(gpu):
    """keyframes 0 and 6; frames 1..5 hang on 0 at depths 1..5, 7..9 on 6."""
    rng = np.random.default_rng(84)
    poses = np.stack([_pose(rng) for _ in range(3)]).astype(np.float32)
    tstamps = np.array([0, 6, 99], np.int64)
    rec = _records_chain(rng, [1, 2, 3, 4, 5, 7, 8, 9])
    out = _check_trajectory(gpu, poses, tstamps, 2, rec, 10)
    assert not np.isnan(out[False]).any()


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_trajectory_long_chain(gpu, order):
    """one chain of depth counter - 1 at counter = 70: seven jumping rounds."""
    rng = np.random.default_rng(85)
    poses = np.stack([_pose(rng) for _ in range(2)]).astype(np.float32)
    tstamps = np.array([0, 500], np.int64)
    rec = _records_chain(rng, range(1, 70))
    if order == "descending":
        rec = rec[::-1]
    elif order == "shuffled":
        rec = [rec[i] for i in rng.permutation(len(rec))]
    out = _check_trajectory(gpu, poses, tstamps, 2, rec, 70, n_as_tensor=(order == "shuffled"))
    assert not np.isnan(out[False]).any()


def test_trajectory_rules(gpu):
    """last record wins, keyframe wins, ignored records, unresolved frames."""
    rng = np.random.default_rng(86)
    poses = np.stack([_pose(rng) for _ in range(3)]).astype(np.float32)
    tstamps = np.array([0, 2, 7], np.int64)  # n = 2: row 2 is not a keyframe
    d = [_pose(rng, rot=0.1, trans=0.2).astype(np.float32) for _ in range(4)]
    rec = [(1, 0, d[0]), (3, 1, d[2]), (1, 0, d[1]),  # two records for 1
           (2, 0, d[3]),                              # 2 is a keyframe
           (3, 3, d[0]), (9, 0, d[0]),                # ignored: t0 >= t1, index >= counter
           (5, 4, d[0]),                              # 4 has nothing, 5 hangs on it
           (7, 6, d[1]), (6, 2, d[2])]                # 7 -> 6 -> keyframe 2 (tstamps row 1)
    out = _check_trajectory(gpu, poses, tstamps, 2, rec, 8)
    assert np.isnan(out[False][[4, 5]]).all() and not np.isnan(out[False][[0, 1, 2, 3, 6, 7]]).any()


def test_trajectory_empty_log(gpu):
    rng = np.random.default_rng(87)
    poses = np.stack([_pose(rng) for _ in range(3)]).astype(np.float32)
    tstamps = np.array([0, 3, 4], np.int64)
    out = _check_trajectory(gpu, poses, tstamps, 3, [], 6)
    assert np.isnan(out[False][[1, 2, 5]]).all()


def test_trajectory_device_n_equals_host_n(gpu):
    from dpvo_amd import frontend

    rng = np.random.default_rng(88)
    poses = np.stack([_pose(rng) for _ in range(6)]).astype(np.float32)
    tstamps = np.array([0, 4, 8, 12, 13, 14], np.int64)
    rec = _records_chain(rng, [1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15])
    dP, dT = _dev(gpu, poses, tstamps)
    delta = _delta(gpu, rec, cap=40)
    n_dev = torch.tensor([4], dtype=torch.int32, device=gpu)
    a = frontend.trajectory(dP, dT, 4, delta, 16)
    b = frontend.trajectory(dP, dT, n_dev, delta, 16)
    for x, y in zip(a, b):
        assert_bit_equal(x.cpu().numpy(), y.cpu().numpy())
    assert a[2].cpu().tolist() == [0, 0]  # rows 4, 5 of poses are beyond n: 13.. follow records


def test_append_delta_equals_hand_filled_log(gpu):
    from dpvo_amd import frontend

    rng = np.random.default_rng(89)
    rec = _records_chain(rng, [1, 2, 3])
    ident = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
    rec.append((4, 3, ident))
    hand = _delta(gpu, rec, cap=5)
    made = (torch.zeros(5, 7, device=gpu), torch.zeros(5, 2, dtype=torch.long, device=gpu),
            torch.zeros(1, dtype=torch.int32, device=gpu))
    for t1, t0, dP in rec[:3]:
        assert frontend.append_delta(made, t1, t0, torch.from_numpy(dP)).item()
    t1 = torch.tensor(4, device=gpu)
    assert frontend.append_delta(made, t1, t1 - 1).item()  # identity, device indices
    for x, y in zip(hand, made):
        assert torch.equal(x, y)
    # a full log keeps its contents and its count
    assert frontend.append_delta(made, 5, 4).item()
    before = [t.clone() for t in made]
    assert not frontend.append_delta(made, 6, 5).item()
    for x, y in zip(before, made):
        assert torch.equal(x, y)
    assert made[2].item() == 5


def test_trajectory_after_keyframe_drop(gpu):
    """DevicePatchGraph.keyframe(delta=...) drops a frame of a synthetic graph and
    records pg.delta; trajectory() then interpolates the dropped frame."""
    from dpvo_amd import frontend, synthetic
    from dpvo_amd.patchgraph import DevicePatchGraph

    N, M, n = 32, 10, 20
    g = synthetic.make_graph(n, M, 4000, seed=5, span=3, num_poses=N, num_patches=N * M)
    pg = DevicePatchGraph(max_edges=4096, DIM=16, device=gpu)
    ix = torch.arange(N * M, device=gpu) // M
    pg.append_factors(ix, g.kk.to(gpu), g.jj.to(gpu))
    dP, dK, dI = g.poses.to(gpu), g.patches.to(gpu), g.intrinsics.to(gpu)
    dT = torch.arange(N, dtype=torch.long, device=gpu)
    st = torch.tensor([n, n * M], dtype=torch.int32, device=gpu)
    log = (torch.zeros(4, 7, device=gpu), torch.zeros(4, 2, dtype=torch.long, device=gpu),
           torch.zeros(1, dtype=torch.int32, device=gpu))
    kf, _ = pg.keyframe(st, dP, dK, dI, M, tstamps=dT, delta=log)
    assert kf.cpu().tolist() == [1, n - 4] and log[2].item() == 1 and pg.errors == 0
    traj, root, info = frontend.trajectory(dP, dT, st[:1], log, n, inverse=True)
    rec = [(int(log[1][0, 0]), int(log[1][0, 1]), log[0][0].cpu().numpy())]
    assert rec[0][:2] == (n - 4, n - 5)
    rt, rr, ri = F.trajectory(dP.cpu().numpy(), dT.cpu().numpy(), n - 1, rec, n, inverse=True)
    np.testing.assert_array_equal(root.cpu().numpy(), rr)
    assert info.cpu().tolist() == ri.tolist() == [0, 0]
    assert_pose_close(traj.cpu().numpy(), rt)
    assert rr[n - 4] == n - 5  # the dropped frame hangs on the keyframe before it
