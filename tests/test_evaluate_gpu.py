"""GPU: trajectory_ate (dpvo_amd/csrc/evaluate.hip, dpvo_amd.evaluation.ate)
against the fp64 numpy restatement of tests/ate_ref.py.

pairs, count and status are compared exactly.  model is held to the project's
Umeyama bar, TOL = 1e-10 of test_ransac_umeyama_gpu.py.  stats are held to 1e-8
absolute: for |x| <= 10 the error of one residual is bounded by
10 dc + 30 dR + sqrt(3) dt = 4.2e-9 at that bar.

Measured on an MI355X over every case below: model within 7.8e-15, stats
within 5.7e-14 of the restatement."""
import numpy as np
import pytest
import torch

import ate_ref as A

pytestmark = pytest.mark.gpu

TOL = 1e-10       # model: tests/test_ransac_umeyama_gpu.py
STATS_TOL = 1e-8  # stats, absolute
_REF = {}


def reference(key, make):
    """(inputs, the restatement's result on exactly those values), computed once."""
    if key not in _REF:
        args = make()
        _REF[key] = (args, A.ate(*args[:4], **args[4]))
    return _REF[key]


def run(gpu, est_xyz, est_t, ref_xyz, ref_t, kw):
    from dpvo_amd.evaluation import ate

    r = ate(torch.from_numpy(np.ascontiguousarray(est_xyz)).to(gpu), est_t, ref_xyz, ref_t, **kw)
    assert r.stats.dtype == torch.float64 and tuple(r.stats.shape) == (8,)
    assert r.model.dtype == torch.float64 and tuple(r.model.shape) == (13,)
    assert r.pairs.dtype == torch.int32 and r.status.dtype == torch.int32
    assert all(t.is_cuda for t in r)
    return r


def check(r, ref, n, m):
    stats, model = r.stats.cpu().numpy(), r.model.cpu().numpy()
    pairs, status = r.pairs.cpu().numpy(), int(r.status.cpu()[0])
    assert pairs.shape == (min(n, m), 2)
    np.testing.assert_array_equal(pairs, ref["pairs"])
    assert status == ref["status"]
    assert stats[7] == ref["stats"][7]
    merr = np.abs(model - ref["model"]).max()
    print(f"status {status} count {stats[7]:.0f} model err {merr:.2e}")
    assert merr <= TOL, merr
    if status != 0:
        assert np.isnan(stats[:7]).all()
        np.testing.assert_array_equal(model, np.concatenate([np.eye(3).reshape(-1), [0, 0, 0, 1]]))
        return
    err = np.abs(stats - ref["stats"])
    print("stats err", err.tolist())
    assert err.max() <= STATS_TOL, err
    assert r.rmse.item() == stats[0]


def _case(n, m, seed, dtype=np.float64, drop=3, **kw):
    def make():
        return A.make_case(n, m, seed, dtype=dtype, drop=drop) + (kw,)
    return reference((n, m, seed, np.dtype(dtype).name, drop, tuple(sorted(kw.items()))), make)


@pytest.mark.parametrize("n,m", [(37, 200), (200, 37)])
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_matches_restatement(gpu, n, m, align, dtype):
    args, ref = _case(n, m, 11, dtype=dtype, align=align)
    assert ref["status"] == 0 and ref["stats"][7] == 34  # three stamps pushed beyond max_diff
    check(run(gpu, *args), ref, n, m)


def test_more_than_one_chunk_and_equal_lengths(gpu):
    """n = m = 1100: the long side is ref, three chunks of 512 stamps in the
    ordered compaction, an even pair count."""
    args, ref = _case(1100, 1100, 12, drop=4)
    assert ref["stats"][7] == 1096
    check(run(gpu, *args), ref, 1100, 1100)


@pytest.mark.parametrize("count", [3, 4, 5, 2, 1, 0])
def test_small_pair_counts(gpu, count):
    """Exactly 3 pairs is the least that aligns; an even and an odd count for the
    median; fewer than 3 set bit 0 with NaN stats and the count still written."""
    def make():
        g = np.random.default_rng(20 + count)
        est_t = np.arange(6.0)
        ref_t = np.concatenate([est_t[:count] + 0.004, est_t[count:] + 0.5, [9.0, 10.0]])
        return g.uniform(-3, 3, (6, 3)), est_t, g.uniform(-3, 3, (8, 3)), ref_t, {}
    args, ref = reference(("small", count), make)
    assert ref["stats"][7] == count and ref["status"] == (0 if count >= 3 else 1)
    check(run(gpu, *args), ref, 6, 8)


def test_hand_written_association(gpu):
    """The cases of test_ate_ref.py on the device: a tie, a duplicate long stamp,
    a pair at exactly max_diff, one just beyond, a repeated long index."""
    def make():
        g = np.random.default_rng(30)
        ref_t = np.array([0.5, 0.5, 1.5, 1.5, 10.0, 20.0, 30.0, 30.0, 40.0])
        est_t = np.array([1.0, 9.75, np.nextafter(19.5, 19), 29.5, 30.25, 40.0, 40.5])
        return (g.uniform(-3, 3, (7, 3)), est_t, g.uniform(-3, 3, (9, 3)), ref_t,
                dict(max_diff=0.5, align=False))
    args, ref = reference("hand", make)
    np.testing.assert_array_equal(ref["pairs"][:6], [[0, 0], [1, 4], [3, 6], [4, 6], [5, 8], [6, 8]])
    check(run(gpu, *args), ref, 7, 9)


def test_collinear_points_set_bit_1(gpu):
    def make():
        ts = np.arange(12.0)
        line = np.outer(ts, [1.0, 0.0, 0.0])  # one non-zero covariance entry: exact rank 1
        return line, ts, 2 * line + 1, ts, {}
    args, ref = reference("line", make)
    assert ref["status"] == 2
    check(run(gpu, *args), ref, 12, 12)
    r = run(gpu, *args[:4], dict(align=False))  # without alignment there is nothing degenerate
    check(r, A.ate(*args[:4], align=False), 12, 12)


@pytest.mark.parametrize("which", ["ref", "est", "nan"])
def test_unsorted_stamps_set_bit_2(gpu, which):
    def make():
        ex, et, rx, rt = A.make_case(37, 200, 13)
        if which == "ref":
            rt[150], rt[151] = rt[151], rt[150]
        elif which == "est":
            et[[0, 36]] = et[[36, 0]]
        else:
            rt[199] = np.nan
        return ex, et, rx, rt, {}
    args, ref = reference(("unsorted", which), make)
    assert ref["status"] & 4 and ref["stats"][7] == 0
    check(run(gpu, *args), ref, 37, 200)


def test_two_runs_are_bit_identical(gpu):
    args, _ = _case(200, 37, 11, align=True)
    a, b = run(gpu, *args), run(gpu, *args)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    big, _ = _case(1100, 1100, 12, drop=4)
    a, b = run(gpu, *big), run(gpu, *big)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))


def test_trajectory_columns_and_validation(gpu):
    """terminate()'s [n, 7] float32 poses go in as they are; refusals are loud."""
    from dpvo_amd.evaluation import ate

    (ex, et, rx, rt, kw), ref = _case(37, 200, 11, dtype=np.float32, align=True)
    traj = torch.zeros(37, 7, device=gpu)
    traj[:, :3] = torch.from_numpy(ex).to(gpu)
    traj[:, 6] = 1
    check(ate(traj, et, rx, rt), ref, 37, 200)
    with pytest.raises(TypeError, match="float32 or float64"):
        ate(traj.half(), et, rx, rt)
    with pytest.raises(RuntimeError, match="est_t"):
        ate(traj, et[:5], rx, rt)
    big = torch.zeros(65537, 3, dtype=torch.float64, device=gpu)
    with pytest.raises(RuntimeError, match="status 3"):
        ate(big, np.arange(65537.0), rx, rt)
