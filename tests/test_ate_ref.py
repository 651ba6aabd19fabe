"""CPU: the ATE restatement (ate_ref.py) on its own, and the TUM text format of
dpvo_amd.evaluation."""
import numpy as np
import pytest

import ate_ref as A
from umeyama_restatement import rotation_of


def _moved(x, R, t, c):
    return c * x @ R.T + t


def test_known_sim3_scores_zero_and_is_recovered():
    g = np.random.default_rng(0)
    x = g.uniform(-5, 5, (60, 3))  # extent 10
    R, t, c = rotation_of([0.3, -0.5, 0.8]), np.array([0.4, -1.1, 2.0]), 0.7
    y = _moved(x, R, t, c)  # |y| <= 0.7 * 5 sqrt(3) + |t|: extent <= 10
    ts = np.arange(60.0)
    r = A.ate(x, ts, y, ts)
    assert r["status"] == 0 and r["stats"][7] == 60
    assert r["stats"][5] < 1e-12 and r["stats"][0] < 1e-12
    np.testing.assert_allclose(r["model"][:9].reshape(3, 3), R, atol=1e-12, rtol=0)
    np.testing.assert_allclose(r["model"][9:12], t, atol=1e-12, rtol=0)
    assert abs(r["model"][12] - c) < 1e-12


def test_without_alignment_the_error_is_the_plain_distance():
    x = np.array([[0.0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]])
    y = x + np.array([3.0, 4.0, 0.0])
    ts = np.arange(4.0)
    r = A.ate(x, ts, y, ts, align=False)
    np.testing.assert_array_equal(r["model"], np.concatenate([np.eye(3).reshape(-1), [0, 0, 0, 1]]))
    np.testing.assert_allclose(r["stats"], [5, 5, 5, 0, 5, 5, 100, 4], atol=1e-15)


def test_statistics_even_and_odd():
    ts = np.arange(5.0)
    y = np.zeros((5, 3))
    x = np.zeros((5, 3))
    x[:, 0] = [1, 2, 4, 8, 16]
    r = A.ate(x, ts, y, ts, align=False)
    np.testing.assert_allclose(r["stats"], [np.sqrt(341 / 5), 6.2, 4, np.sqrt(341 / 5 - 6.2 ** 2),
                                            1, 16, 341, 5], rtol=1e-12)
    r = A.ate(x[:4], ts[:4], y[:4], ts[:4], align=False)
    assert r["stats"][2] == 3.0 and r["stats"][7] == 4  # the mean of the two middle values


# ---- association, written out by hand ------------------------------------------------------
def test_est_longer_than_ref():
    est_t = [0.0, 1.0, 2.0, 3.0, 4.0]
    ref_t = [1.004, 2.9, 3.999]
    np.testing.assert_array_equal(A.associate(est_t, ref_t), [[1, 0], [4, 2]])


def test_ref_longer_than_est():
    est_t = [1.004, 2.9, 3.999]
    ref_t = [0.0, 1.0, 2.0, 3.0, 4.0]
    np.testing.assert_array_equal(A.associate(est_t, ref_t), [[0, 1], [2, 4]])


def test_equal_lengths_take_ref_as_the_long_side():
    # n == m: the long side is ref, pairs run in est order
    np.testing.assert_array_equal(A.associate([0.0, 1.0], [1.0, 5.0]), [[1, 0]])


def test_tie_goes_to_the_lower_index():
    # 0.5 and 1.5 are exact: |dt| = 0.25 on both sides
    np.testing.assert_array_equal(A.associate([0.75], [0.5, 1.0, 2.0], max_diff=0.25), [[0, 0]])
    np.testing.assert_array_equal(A.associate([1.0], [0.5, 0.5, 1.5, 1.5], max_diff=1.0), [[0, 0]])


def test_pair_at_exactly_max_diff_is_kept_and_just_beyond_is_dropped():
    md = 0.25
    ref_t = [0.0, 10.0, 20.0]
    np.testing.assert_array_equal(A.associate([10.25], ref_t, md), [[0, 1]])
    np.testing.assert_array_equal(A.associate([9.75], ref_t, md), [[0, 1]])
    assert len(A.associate([np.nextafter(10.25, 11)], ref_t, md)) == 0
    assert len(A.associate([np.nextafter(9.75, 9)], ref_t, md)) == 0


def test_a_long_index_may_repeat():
    np.testing.assert_array_equal(A.associate([0.999, 1.001, 5.0], [0.0, 1.0, 2.0, 3.0]),
                                  [[0, 1], [1, 1]])


def test_pairs_padding_and_status_bits():
    ts = np.arange(4.0)
    x = np.random.default_rng(1).uniform(-1, 1, (4, 3))
    r = A.ate(x, ts, x, [0.0, 1.0, 2.5, 3.5])
    assert r["status"] == 1 and r["stats"][7] == 2 and np.isnan(r["stats"][:7]).all()
    np.testing.assert_array_equal(r["pairs"], [[0, 0], [1, 1], [-1, -1], [-1, -1]])
    line = np.outer(np.arange(4.0), [1.0, 0.0, 0.0])  # one non-zero covariance entry: exact rank 1
    r = A.ate(line, ts, 2 * line, ts)
    assert r["status"] == 2 and r["stats"][7] == 4 and np.isnan(r["stats"][:7]).all()
    r = A.ate(x, ts, x, [0.0, 2.0, 1.0, 3.0])
    assert r["status"] & 4 and r["stats"][7] == 0 and (r["pairs"] == -1).all()


def test_make_case_is_what_the_gpu_tests_want():
    for n, m in ((37, 200), (200, 37)):
        ex, et, rx, rt = A.make_case(n, m, seed=3)
        assert ex.shape == (n, 3) and rx.shape == (m, 3)
        assert A.is_sorted(et) and A.is_sorted(rt)
        assert np.abs(ex).max() <= 10 and np.abs(rx).max() <= 10
        r = A.ate(ex, et, rx, rt)
        assert r["status"] == 0 and r["stats"][7] == 37 - 3
        assert 3e-3 < r["stats"][0] < 5e-2  # noise 1e-2 per axis


# ---- TUM files ------------------------------------------------------------------------------
def test_tum_round_trip(tmp_path):
    from dpvo_amd.evaluation import read_tum, write_tum

    g = np.random.default_rng(2)
    poses = g.standard_normal((5, 7))
    ts = 1403636579.763555527 + np.arange(5.0)
    write_tum(tmp_path / "t.txt", poses, ts)
    t2, p2 = read_tum(tmp_path / "t.txt")
    np.testing.assert_array_equal(t2, ts)
    np.testing.assert_array_equal(p2, poses)


def test_read_tum_comments_commas_and_short_lines(tmp_path):
    from dpvo_amd.evaluation import read_tum

    p = tmp_path / "gt.txt"
    p.write_text("# timestamp tx ty tz qx qy qz qw\n1.5 1 2 3 0 0 0 1\n\n2.5,4,5,6,0,0,0,1  # x\n")
    t, poses = read_tum(p)
    assert t.tolist() == [1.5, 2.5] and poses[1].tolist() == [4, 5, 6, 0, 0, 0, 1]
    p.write_text("1.5 1 2 3\n")
    with pytest.raises(ValueError, match="8 numbers"):
        read_tum(p)
