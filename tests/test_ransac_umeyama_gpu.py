"""The RANSAC-Umeyama estimator on the device (dpvo_amd/csrc/ransac.hip,
cuda_ba.ransac_umeyama, loop_closure.ransac_umeyama) against the fp64 numpy
restatement of tests/umeyama_restatement.py.

Counts, stop index, winner and mask are compared exactly: every case keeps all
its distances at least 1e-9 away from the threshold (asserted), and fp64
rounding of a distance of magnitude <= 40 is about 1e-14.  R, t, s are
compared to 1e-10 absolute: the bound is the worst-case fp64 summation error
N eps |x|^2 at N = 2048 and |x| <= 20 (2048 * 2.2e-16 * 400 = 1.8e-10), not a
measured figure.

Measured on an MI355X, over the five cases and both input dtypes: R / t / s
within 8.0e-15 of the restatement, the quaternion within 4.4e-16.
"""
import numpy as np
import pytest
import torch

import umeyama_restatement as U

TOL = 1e-10
DTYPES = {"f64": torch.float64, "f32": torch.float32}
_REF = {}


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    return dpvo_amd.load_extension("cuda_ba")


@pytest.fixture(scope="module")
def lc(gpu):
    from dpvo_amd import loop_closure

    return loop_closure


def reference(case, dt, early_exit=100):
    """(src, dst in the numpy dtype `dt`, samples, the restatement's result on
    exactly those values), computed once."""
    key = (case, dt, early_exit)
    if key not in _REF:
        src, dst, samples = U.make_case(*case)
        src, dst = src.astype(dt), dst.astype(dt)
        _REF[key] = (src, dst, samples, U.ransac_umeyama(src, dst, samples, early_exit=early_exit))
    return _REF[key]


def run(cb, gpu, src, dst, samples, threshold=0.1, early_exit=100):
    model, info, mask, counts = cb.ransac_umeyama(
        torch.from_numpy(src).to(gpu), torch.from_numpy(dst).to(gpu),
        torch.from_numpy(np.asarray(samples)).to(gpu), threshold, early_exit, return_counts=True)
    return model.cpu().numpy(), info.cpu().tolist(), mask.cpu().numpy(), counts.cpu().numpy()


def check_model(model, ref, tol=TOL):
    R, t, s = model[:9].reshape(3, 3), model[9:12], model[12]
    err = max(np.abs(R - ref["R"]).max(), np.abs(t - ref["t"]).max(), abs(s - ref["s"]))
    q = U.quaternion_of(ref["R"])
    qerr = min(np.abs(model[16:20] - q).max(), np.abs(model[16:20] + q).max())
    assert err <= tol and qerr <= tol, (err, qerr)
    assert np.array_equal(model[13:16], t) and model[20] == s and model[19] >= 0
    assert abs(np.linalg.det(R) - 1) < 1e-12
    return err, qerr


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", list(U.CASES), ids=lambda c: "N%d-H%d-seed%d" % c[:3])
def test_matches_restatement(cb, lc, gpu, case, dtype):
    dt = np.float64 if dtype == "f64" else np.float32
    src, dst, samples, ref = reference(case, dt)
    assert ref["min_margin"] >= 1e-9 and ref["status"] == 0
    model, info, mask, counts = run(cb, gpu, src, dst, samples)
    assert np.array_equal(counts, ref["counts"])
    assert info == [ref["num_inliers"], ref["winner"], ref["stop"], 0]
    assert np.array_equal(mask, ref["mask"])
    err, qerr = check_model(model, ref)
    print(case, dtype, "max abs error of R / t / s", err, "of the quaternion", qerr)

    # the Python surface: the same numbers in the input dtype
    est = lc.ransac_umeyama(torch.from_numpy(src).to(gpu), torch.from_numpy(dst).to(gpu),
                            samples=torch.from_numpy(samples).to(gpu))
    tdt = DTYPES[dtype]
    assert est.R.shape == (3, 3) and est.t.shape == (3,) and est.s.shape == ()
    assert est.sim3.shape == (8,) and est.mask.dtype == torch.bool
    assert all(x.dtype == tdt for x in (est.R, est.t, est.s, est.sim3))
    assert (int(est.num_inliers), int(est.hypothesis), int(est.status)) == (info[0], info[1], 0)
    assert np.array_equal(est.mask.cpu().numpy(), ref["mask"])
    want = torch.from_numpy(model).to(tdt)  # f32: the fp64 model rounded once
    got = torch.cat([est.R.reshape(-1), est.t, est.s[None], est.sim3]).cpu()
    assert torch.equal(got, want)
    q = U.quaternion_of(ref["R"])
    sim3 = est.sim3.double().cpu().numpy()
    sim3_ref = np.concatenate([ref["t"], q if np.dot(q, sim3[3:7]) > 0 else -q, [ref["s"]]])
    bound = TOL if dtype == "f64" else 2.0 ** -24 * np.maximum(1.0, np.abs(sim3_ref)) + TOL
    assert (np.abs(sim3 - sim3_ref) <= bound).all()


@pytest.mark.gpu
def test_two_calls_are_bit_identical(cb, gpu):
    src, dst, samples, _ = reference((2048, 400, 10, 0.6), np.float64)
    a = run(cb, gpu, src, dst, samples)
    b = run(cb, gpu, src, dst, samples)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.gpu
def test_three_points(cb, gpu):
    """N = 3, H = 1: exact fit, refit over the same three points; a mirrored
    cloud is still answered with a proper rotation."""
    R, t, s = U.TRUTH
    src = np.array([[0.5, -1.0, 2.0], [1.5, 0.25, 3.0], [-0.75, 1.0, 5.0]])
    dst = s * src @ R.T + t
    smp = np.array([[0, 1, 2]])
    model, info, mask, counts = run(cb, gpu, src, dst, smp)
    assert info == [3, 0, 0, 0] and mask.all() and counts.tolist() == [3]
    check_model(model, dict(R=R, t=t, s=s), tol=1e-12)

    mirrored = dst * np.array([1.0, 1.0, -1.0])
    ref = U.ransac_umeyama(src, mirrored, smp)
    model, info, mask, counts = run(cb, gpu, src, mirrored, smp)
    assert info == [ref["num_inliers"], 0, 0, 0] and counts.tolist() == ref["counts"].tolist()
    assert np.array_equal(mask, ref["mask"])
    assert abs(np.linalg.det(model[:9].reshape(3, 3)) - 1) < 1e-12
    check_model(model, ref, tol=1e-12)


@pytest.mark.gpu
def test_degenerate_samples(cb, gpu):
    # the rank test is absolute (2.2e-16), so the collinear points lie along
    # coordinate axes: their covariance has one non-zero entry, exactly
    src, dst, samples = U.make_case(90, 64, 8, 0.4)
    src, dst, samples = src.copy(), dst.copy(), samples.copy()
    src[[10, 11, 12]] = [[0, 0, 1], [1, 0, 1], [2, 0, 1]]
    dst[[10, 11, 12]] = [[1, 0, 0], [1, 2, 0], [1, 4, 0]]
    samples[2] = [10, 11, 12]
    ref = U.ransac_umeyama(src, dst, samples)
    assert ref["counts"][2] == -1 and ref["min_margin"] >= 1e-9 and ref["winner"] != 2
    model, info, mask, counts = run(cb, gpu, src, dst, samples)
    assert counts[2] == -1 and np.array_equal(counts, ref["counts"])
    assert info == [ref["num_inliers"], ref["winner"], ref["stop"], 0]
    assert np.array_equal(mask, ref["mask"])
    check_model(model, ref)

    # every sample collinear: status 1, the identity, no inliers
    line = np.outer(np.arange(40.0), [0.5, 0.0, 0.0])
    smp = np.array([[0, 1, 2], [5, 9, 30], [39, 3, 17]])
    assert U.ransac_umeyama(line, line, smp)["status"] == 1
    model, info, mask, counts = run(cb, gpu, line, line, smp)
    assert counts.tolist() == [-1, -1, -1] and info == [0, -1, 2, 1] and not mask.any()
    ident = np.concatenate([np.eye(3).ravel(), [0, 0, 0, 1], [0, 0, 0], [0, 0, 0, 1], [1]])
    assert np.array_equal(model, ident)

    # a valid sample (a triangle 1e-7 high: second singular value 2.2e-15)
    # whose 200 inliers are collinear but for one point (4.5e-17): status 2
    pts = np.zeros((200, 3))
    pts[:, 0] = 0.1 * np.arange(200)
    pts[1, 1] = 1e-7
    ref = U.ransac_umeyama(pts, pts.copy(), smp[:1], early_exit=1000)
    assert ref["status"] == 2 and ref["num_inliers"] == 200
    model, info, mask, counts = run(cb, gpu, pts, pts.copy(), smp[:1], early_exit=1000)
    assert counts.tolist() == [200] and info == [200, 0, 0, 2] and mask.all()
    assert np.array_equal(model, ident)


@pytest.mark.gpu
def test_early_exit_disabled(cb, gpu):
    """early_exit >= N: the loop runs to the end and finds the hypothesis the
    default early exit never sees."""
    case = (2048, 400, 10, 0.6)
    src, dst, samples, ref = reference(case, np.float64, early_exit=2048)
    assert (ref["winner"], ref["num_inliers"], ref["stop"]) == (10, 834, 399)
    model, info, mask, counts = run(cb, gpu, src, dst, samples, early_exit=2048)
    assert info == [834, 10, 399, 0] and np.array_equal(mask, ref["mask"])
    check_model(model, ref)


@pytest.mark.gpu
def test_drawn_samples(lc, gpu):
    N, H = 257, 400
    g = torch.Generator(device=gpu)
    a = lc.draw_samples(N, H, gpu, g.manual_seed(5))
    b = lc.draw_samples(N, H, gpu, g.manual_seed(5))
    c = lc.draw_samples(N, H, gpu, g.manual_seed(6))
    assert a.shape == (H, 3) and torch.equal(a, b) and not torch.equal(a, c)
    s = a.sort(dim=1).values
    assert int(a.min()) >= 0 and int(a.max()) < N
    assert bool((s[:, 0] < s[:, 1]).all()) and bool((s[:, 1] < s[:, 2]).all())
    assert a.unique().numel() > N // 2  # spread over the cloud, not a few indices
    src, dst, _, _ = reference((257, 64, 7, 0.4), np.float64)
    est = lc.ransac_umeyama(torch.from_numpy(src).to(gpu), torch.from_numpy(dst).to(gpu),
                            iterations=H, generator=g.manual_seed(5))
    assert int(est.status) == 0 and int(est.num_inliers) > 100
    print("drawn samples: s", float(est.s), "inliers", int(est.num_inliers),
          "hypothesis", int(est.hypothesis))
    assert abs(float(est.s) - 1.7) <= 1e-2  # the restatement's own refit is 1.4e-4 off


@pytest.mark.gpu
def test_graph_capture(cb, gpu):
    """One call captured (its two kernels on one stream), the input buffers
    overwritten with another case, replayed: the eager result of that case."""
    first = U.make_case(90, 64, 8, 0.4)
    second = U.make_case(90, 64, 12, 0.4)
    dev = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    src, dst, smp = dev(first[0]), dev(first[1]), dev(first[2]).int()

    def call():
        return cb.ransac_umeyama(src, dst, smp, 0.1, 100, check_samples=False, return_counts=True)

    eager_first = [t.clone() for t in call()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(out, eager_first):
        assert torch.equal(got, want)
    src.copy_(dev(second[0]))
    dst.copy_(dev(second[1]))
    smp.copy_(dev(second[2]).int())
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    eager_second = call()
    assert not torch.equal(eager_second[0], eager_first[0])
    for got, want in zip(replayed, eager_second):
        assert torch.equal(got, want)


@pytest.mark.gpu
def test_validation(cb, lc, gpu):
    src = torch.rand(20, 3, device=gpu, dtype=torch.float64)
    smp = torch.tensor([[0, 1, 2], [3, 4, 19]], device=gpu)
    assert cb.ransac_umeyama(src, src, smp, 0.1, 100)[1][3] == 0
    name = "ransac_umeyama"
    with pytest.raises(RuntimeError, match=name):
        cb.ransac_umeyama(src.cpu(), src.cpu(), smp.cpu(), 0.1, 100)
    with pytest.raises(RuntimeError, match=name + ".*dtype"):
        cb.ransac_umeyama(src, src.float(), smp, 0.1, 100)
    with pytest.raises(RuntimeError, match=name):
        cb.ransac_umeyama(src.half(), src.half(), smp, 0.1, 100)
    with pytest.raises(RuntimeError, match=name + r".*\[N, 3\]"):
        cb.ransac_umeyama(src[:, :2], src[:, :2], smp, 0.1, 100)
    with pytest.raises(RuntimeError, match=name + r".*\[N, 3\]"):
        cb.ransac_umeyama(src, src[:10], smp, 0.1, 100)
    with pytest.raises(RuntimeError, match=name + r".*\[H, 3\]"):
        cb.ransac_umeyama(src, src, smp[:, :2], 0.1, 100)
    with pytest.raises(RuntimeError, match=name + ".*N >= 3"):
        cb.ransac_umeyama(src[:2], src[:2], smp, 0.1, 100)
    with pytest.raises(RuntimeError, match=name + ".*threshold"):
        cb.ransac_umeyama(src, src, smp, 0.0, 100)
    for bad in (20, -1):
        s2 = smp.clone()
        s2[1, 2] = bad
        with pytest.raises(RuntimeError, match=name + ".*out of range"):
            cb.ransac_umeyama(src, src, s2, 0.1, 100)
        with pytest.raises(RuntimeError, match=name + ".*out of range"):
            lc.ransac_umeyama(src, src, samples=s2)
        # unchecked, the sample is only a hypothesis without a model
        _, info, _, counts = cb.ransac_umeyama(src, src, s2, 0.1, 100, check_samples=False,
                                               return_counts=True)
        assert counts.tolist() == [20, -1] and info.tolist() == [20, 0, 1, 0]
