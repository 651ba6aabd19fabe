"""CPU: the vectorised restatement of the descriptor matcher (match_ref.py)
against the definition written as a plain double loop, on sizes up to 9 x 7."""
import numpy as np
import pytest

import match_ref as MR


def _ternary(rng, n, d):
    return (rng.integers(-1, 2, size=(n, d)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("N0,N1,D", [(1, 1, 4), (1, 7, 4), (7, 1, 4), (5, 5, 8), (9, 7, 4), (9, 7, 12)])
@pytest.mark.parametrize("ratio,max_dist", [(0.8, np.inf), (1.0, np.inf), (0.75, 0.375), (1.0, 0.25)])
def test_restatement_equals_loops(N0, N1, D, ratio, max_dist):
    hits = 0
    for seed in range(6):
        rng = np.random.default_rng(1000 * seed + 17 * N0 + N1 + D)
        a, b = _ternary(rng, N0, D), _ternary(rng, N1, D)
        if N0 > 2 and N1 > 2:  # duplicates: ties in both directions
            b[1] = b[0]
            a[2] = a[1]
            b[2] = a[0]
        ref = MR.match_ref(a, b, ratio, max_dist)
        p0, p1, pairs = MR.match_loops(a, b, ratio, max_dist)
        assert ref["partner0"].tolist() == p0 and ref["partner1"].tolist() == p1
        k = ref["count"]
        assert k == len(pairs)
        assert [tuple(m) for m in ref["matches"][:k].tolist()] == [(i, j) for i, j, _ in pairs]
        np.testing.assert_array_equal(ref["dist2"][:k], np.array([d for _, _, d in pairs], np.float32))
        assert (ref["matches"][k:] == -1).all() and (ref["dist2"][k:] == -1).all()
        hits += k
    if ratio == 1.0 and max_dist == np.inf:
        assert hits > 0  # mutual nearest neighbours always exist without the two tests


def test_ties_take_the_lower_index_and_second_is_the_tied_value():
    a = np.array([[1, 0, 0, 0]], np.float32) / 8
    b = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]], np.float32) / 8
    ref = MR.match_ref(a, b, ratio=1.0)
    j, d, s = ref["row"]
    assert (j[0], d[0], s[0]) == (1, 0.0, 0.0)
    assert ref["partner0"].tolist() == [1] and ref["partner1"].tolist() == [-1, 0, -1]
    # with a ratio below 1 the tie at d2 = 0 still passes: 0 <= r2 * 0
    assert MR.match_ref(a, b, ratio=0.5)["count"] == 1
    # one valid column: the second-best is +inf and the ratio test passes
    one = MR.match_ref(a, b, ratio=0.1, n1=1)
    assert one["row"][2][0] == np.inf and one["partner0"].tolist() == [0]


def test_row_limits_ignore_nan_rows():
    rng = np.random.default_rng(3)
    a, b = _ternary(rng, 6, 8), _ternary(rng, 7, 8)
    full = MR.match_ref(a[:4], b[:5], ratio=1.0)
    a[4:], b[5:] = np.nan, np.nan
    cut = MR.match_ref(a, b, ratio=1.0, n0=4, n1=5)
    assert cut["partner0"][:4].tolist() == full["partner0"].tolist()
    assert (cut["partner0"][4:] == -1).all() and (cut["partner1"][5:] == -1).all()
    assert cut["count"] == full["count"] and cut["matches"].shape == (6, 2)
