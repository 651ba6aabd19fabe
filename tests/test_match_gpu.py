"""GPU: dpvo_amd.long_term.match_descriptors (csrc/match.hip) against the numpy
restatement tests/match_ref.py.

Exact inputs: every entry is in {-1, 0, 1} / 8, so products are multiples of
1/64 and every dot product, norm and d2 is exact in fp32 whatever the order of
the sums: the kernel must equal the restatement bit for bit.  The cases run
with ratio 0.75 (r2 = 0.5625 = 9/16) and max_dist 0.375 (max_dist^2 = 9/64),
both exact, and carry planted rows (cases with N >= 10, D >= 32):

  rows 0, 2, 3 / columns 0, 1, 2   duplicates: ties go to the lower index
  row 4 / columns 4, 5             d2 = 9/64, second 16/64: exactly r2 * second
  row 6 / column 6                 d2 = 9/64: exactly max_dist^2
  row 7 / column 7                 d2 = 10/64: just beyond max_dist^2
  row 8 / columns 8, 9             d2 = 9/64, second 15/64: just fails the ratio
"""
import numpy as np
import pytest
import torch

import match_ref as MR

pytestmark = pytest.mark.gpu

RATIO, MAX_DIST = 0.75, 0.375
CASES = [(1, 1, 4), (1, 7, 4), (63, 65, 32), (64, 64, 128), (130, 257, 128), (2048, 2048, 128)]


def _step(row, k, rng):
    """`row` with k of its components moved by one step of 1/8 (d2 = k / 64)."""
    out = row.copy()
    idx = rng.permutation(len(row))[:k]
    out[idx] = np.where(row[idx] > 0, row[idx] - 0.125, row[idx] + 0.125)
    return out


def exact_case(N0, N1, D, seed=0):
    rng = np.random.default_rng(seed + 31 * N0 + 7 * N1 + D)
    a = (rng.integers(-1, 2, size=(N0, D)) / 8.0).astype(np.float32)
    b = (rng.integers(-1, 2, size=(N1, D)) / 8.0).astype(np.float32)
    if N1 >= 2:
        b[1] = b[0]
    if N0 >= 10 and N1 >= 10 and D >= 32:
        b[0] = b[1] = a[0]
        a[3] = a[2]
        b[2] = _step(a[2], 1, rng)
        b[4], b[5] = _step(a[4], 9, rng), _step(a[4], 16, rng)
        b[6] = _step(a[6], 9, rng)
        b[7] = _step(a[7], 10, rng)
        b[8], b[9] = _step(a[8], 9, rng), _step(a[8], 15, rng)
    return a, b


def _run(gpu, a, b, dtype=torch.float32, **kw):
    from dpvo_amd.long_term import match_descriptors

    ta = torch.from_numpy(a).to(gpu, dtype)
    tb = torch.from_numpy(b).to(gpu, dtype)
    return match_descriptors(ta, tb, **kw)


def _assert_equal(got, ref, what=""):
    np.testing.assert_array_equal(got.partner0.cpu().numpy(), ref["partner0"], what)
    np.testing.assert_array_equal(got.partner1.cpu().numpy(), ref["partner1"], what)
    np.testing.assert_array_equal(got.matches.cpu().numpy(), ref["matches"], what)
    assert got.dist2.dtype == torch.float32 and got.count.dtype == torch.int32
    np.testing.assert_array_equal(got.dist2.cpu().numpy().view(np.uint32),
                                  ref["dist2"].view(np.uint32), what)
    assert int(got.count) == ref["count"], what


def _assert_consistent(got, N0, N1):
    p0, p1 = got.partner0.cpu().numpy(), got.partner1.cpu().numpy()
    m, d, k = got.matches.cpu().numpy(), got.dist2.cpu().numpy(), int(got.count)
    assert p0.shape == (N0,) and p1.shape == (N1,) and m.shape == (min(N0, N1), 2)
    assert d.shape == (min(N0, N1),)
    assert (m[k:] == -1).all() and (d[k:] == -1).all()
    assert k == int((p0 >= 0).sum()) == int((p1 >= 0).sum())
    assert (np.diff(m[:k, 0]) > 0).all()
    np.testing.assert_array_equal(m[:k, 0], np.nonzero(p0 >= 0)[0])
    np.testing.assert_array_equal(m[:k, 1], p0[p0 >= 0])
    np.testing.assert_array_equal(p1[m[:k, 1]], m[:k, 0])
    assert (d[:k] >= 0).all()


@pytest.mark.parametrize("N0,N1,D", CASES)
def test_exact_inputs_bit_for_bit(gpu, N0, N1, D):
    a, b = exact_case(N0, N1, D)
    ref = MR.match_ref(a, b, RATIO, MAX_DIST)
    if N0 >= 10 and N1 >= 10 and D >= 32:  # the planted rows do what the docstring says
        rj, rd, rs = ref["row"]
        assert rj[0] == 0 and rd[0] == 0 and rs[0] == 0 and ref["partner0"][0] == 0
        assert ref["col"][0][2] == 2 and ref["partner0"][2] == -1 and ref["partner0"][3] == -1
        assert rd[4] == ref["r2"] * rs[4] and ref["partner0"][4] == 4
        assert rd[6] == ref["md2"] and ref["partner0"][6] == 6
        assert rj[7] == 7 and rd[7] == np.float32(10 / 64) and ref["partner0"][7] == -1
        assert rj[8] == 8 and rs[8] == np.float32(15 / 64) and ref["partner0"][8] == -1
    dtypes = (torch.float32,) if N0 == 2048 else (torch.float32, torch.float16)
    for dtype in dtypes:
        got = _run(gpu, a, b, dtype, ratio=RATIO, max_dist=MAX_DIST)
        _assert_equal(got, ref, f"{dtype}")
        _assert_consistent(got, N0, N1)
    # without the two tests: plain mutual nearest neighbours, many ties
    got = _run(gpu, a, b, ratio=1.0)
    _assert_equal(got, MR.match_ref(a, b, 1.0), "ratio 1")
    _assert_consistent(got, N0, N1)
    again = _run(gpu, a, b, ratio=1.0)
    for x, y in zip(got, again):  # determinism: two runs are bit-equal
        assert torch.equal(x, y)


@pytest.mark.parametrize("N0,N1,D,n0,n1", [(63, 65, 32, 40, 33), (130, 257, 128, 64, 129),
                                           (130, 257, 128, 65, 1), (64, 64, 128, 0, 10)])
def test_row_limits(gpu, N0, N1, D, n0, n1):
    """Rows at or beyond the limit hold NaN and take no part, with the limit
    as a Python int and as an int32 device scalar (also one beyond the rows
    present, which is clamped)."""
    a, b = exact_case(N0, N1, D)
    a[n0:], b[n1:] = np.nan, np.nan
    ref = MR.match_ref(a, b, RATIO, MAX_DIST, n0=n0, n1=n1)
    assert ref["count"] > 0 or n0 == 0
    got = _run(gpu, a, b, ratio=RATIO, max_dist=MAX_DIST, n0=n0, n1=n1)
    _assert_equal(got, ref, "int limits")
    _assert_consistent(got, N0, N1)
    d0 = torch.tensor([n0], dtype=torch.int32, device=gpu)
    d1 = torch.tensor([n1], dtype=torch.int32, device=gpu)
    got = _run(gpu, a, b, torch.float16, ratio=RATIO, max_dist=MAX_DIST, n0=d0, n1=d1)
    _assert_equal(got, ref, "device limits")
    a2, b2 = exact_case(N0, N1, D)
    big = torch.tensor([1 << 20], dtype=torch.int32, device=gpu)
    _assert_equal(_run(gpu, a2, b2, ratio=RATIO, max_dist=MAX_DIST, n0=big, n1=N1 + 5),
                  MR.match_ref(a2, b2, RATIO, MAX_DIST), "clamped limits")


def random_case(N0, N1, D, planted, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((N0, D))
    b = rng.standard_normal((N1, D))
    ia, ib = rng.permutation(N0)[:planted], rng.permutation(N1)[:planted]
    # noise of squared norm ~0.2 against unit descriptors
    b[ib] = a[ia] / np.linalg.norm(a[ia], axis=1, keepdims=True) * np.sqrt(D) \
        + rng.standard_normal((planted, D)) * np.sqrt(0.2)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a.astype(np.float32), b.astype(np.float32)


def unsure(best_d, second_d, r2, md2, tol=1e-5):
    """Rows whose decision has a margin below tol (relative) in fp64: best
    against second-best, the ratio test, the distance cap."""
    tiny = 1e-300
    m1 = (second_d - best_d) / np.maximum(second_d, tiny)
    m2 = np.abs(best_d - r2 * second_d) / np.maximum(r2 * second_d, tiny)
    m3 = np.abs(best_d - md2) / max(md2, tiny)
    with np.errstate(invalid="ignore"):
        return (m1 < tol) | (m2 < tol) | (m3 < tol)


def excused(ref, tol=1e-5):
    """(rows, columns) that may be left out: an unsure decision of their own,
    or of the partner their own (sure) best points at."""
    rj, rd, rs = ref["row"]
    ci, cd, cs = ref["col"]
    r2, md2 = float(ref["r2"]), float(ref["md2"])
    ur, uc = unsure(rd, rs, r2, md2, tol), unsure(cd, cs, r2, md2, tol)
    return ur | uc[rj], uc | ur[ci]


@pytest.mark.parametrize("N0,N1,D,planted,seed", [(2048, 2048, 128, 200, 0), (130, 257, 128, 100, 0)])
def test_random_inputs_against_fp64(gpu, N0, N1, D, planted, seed):
    """Unit-normalised Gaussian descriptors with planted noisy correspondences,
    ratio 0.8, max_dist 0.6, against the fp64 restatement.  A row or column is
    left out only where a decision margin is below 1e-5 relative in fp64; at
    most 1 % may be.  Observed on the CPU with seed 0: 4 of 2048 rows and 1 of
    2048 columns (0.2 % / 0.05 %) at 2048 x 2048 x 128, none at 130 x 257 x 128
    (the counts are printed)."""
    a, b = random_case(N0, N1, D, planted, seed)
    ref = MR.match_ref(a, b, 0.8, 0.6, dtype=np.float64)
    er, ec = excused(ref)
    print(f"excused rows {int(er.sum())} / {N0}, columns {int(ec.sum())} / {N1}; "
          f"matches {ref['count']}")
    assert er.mean() <= 0.01 and ec.mean() <= 0.01
    assert ref["count"] >= planted // 2
    got = _run(gpu, a, b, ratio=0.8, max_dist=0.6)
    _assert_consistent(got, N0, N1)
    p0, p1 = got.partner0.cpu().numpy(), got.partner1.cpu().numpy()
    np.testing.assert_array_equal(p0[~er], ref["partner0"][~er])
    np.testing.assert_array_equal(p1[~ec], ref["partner1"][~ec])
    # d2 of the pairs both agree on.  Worst case of three fp32 fma chains of length D at unit
    # norm: D 2^-24 (|a|^2 + |b|^2 + 2 |a| |b|) = 4 D 2^-24
    m, k = got.matches.cpu().numpy(), int(got.count)
    same = ref["partner0"][m[:k, 0]] == m[:k, 1]
    d_ref = ref["row"][1][m[:k, 0]]
    err = np.abs(got.dist2.cpu().numpy()[:k] - d_ref)[same].max()
    print(f"max |d2 - fp64| = {err:.3g}")
    assert err <= 4 * D * 2.0 ** -24


def test_graph_replay(gpu):
    """No host sync: the call is captured into a graph and replayed on new
    descriptors and a new device row limit."""
    from dpvo_amd.long_term import match_descriptors

    a, b = exact_case(130, 257, 128)
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    lim = torch.tensor([130], dtype=torch.int32, device=gpu)
    match_descriptors(ta, tb, RATIO, MAX_DIST, n0=lim)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = match_descriptors(ta, tb, RATIO, MAX_DIST, n0=lim)
    a2, b2 = exact_case(130, 257, 128, seed=5)
    ta.copy_(torch.from_numpy(a2))
    tb.copy_(torch.from_numpy(b2))
    lim.fill_(77)
    g.replay()
    torch.cuda.synchronize()
    _assert_equal(out, MR.match_ref(a2, b2, RATIO, MAX_DIST, n0=77), "replay")
