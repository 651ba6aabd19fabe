"""CPU: the numpy restatement of Umeyama / RANSAC (tests/umeyama_restatement.py)
checks itself, the fixed cases of the GPU tests have the properties those
tests rely on, and dpvo_ransac_umeyama validates its arguments on the host
before any launch (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import umeyama_restatement as U


@pytest.fixture(scope="module")
def results():
    return {k: U.ransac_umeyama(*U.make_case(*k)) for k in U.CASES}


def test_noiseless_recovers_truth():
    src, dst, samples = U.make_case(64, 4, 3, 0.0, noise=0.0)
    R, t, s = U.TRUTH
    assert abs(np.linalg.det(R) - 1) < 1e-14 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    fR, ft, fs = U.umeyama_alignment(src, dst)
    assert np.abs(fR - R).max() < 1e-12 and np.abs(ft - t).max() < 1e-12 and abs(fs - s) < 1e-12
    # three points are enough, and the rank-2 covariance still gives a proper rotation
    fR, ft, fs = U.umeyama_alignment(src[:3], dst[:3])
    assert np.abs(fR - R).max() < 1e-12 and np.abs(ft - t).max() < 1e-12 and abs(fs - s) < 1e-12
    out = U.ransac_umeyama(src, dst, samples)
    assert out["status"] == 0 and out["num_inliers"] == 64 and out["winner"] == 0
    assert out["mask"].all() and (out["counts"] == 64).all()
    assert np.abs(out["R"] - R).max() < 1e-12 and abs(out["s"] - s) < 1e-12
    q = U.quaternion_of(R)
    assert q[3] >= 0 and abs(np.linalg.norm(q) - 1) < 1e-14
    x, y, z, w = q
    assert np.abs(np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
                  - R).max() < 1e-14


def test_degenerate_inputs_have_no_model():
    # the rank test is absolute (eps), so a line counts as degenerate only when
    # its second singular value is below 2.2e-16: along an axis the covariance
    # has one non-zero entry and the others are exact zeros
    line = np.outer(np.arange(5.0), [1.0, 0.0, 0.0])
    assert U.umeyama_alignment(line, 2 * line + 1) is None
    assert U.umeyama_alignment(line[:3], line[:3, [1, 0, 2]] + [1.0, 0.0, 0.0]) is None
    out = U.ransac_umeyama(line, line, np.array([[0, 1, 2], [2, 3, 4]]))
    assert out["status"] == 1 and out["winner"] == -1 and out["num_inliers"] == 0
    assert (out["counts"] == -1).all() and out["R"] is None


@pytest.mark.parametrize("case", list(U.CASES), ids=lambda c: "N%d-H%d-seed%d" % c[:3])
def test_case_table(results, case):
    out = results[case]
    stop, winner, inliers = U.CASES[case]
    counts = out["counts"]
    print(case, "stop", out["stop"], "winner", out["winner"], "inliers", out["num_inliers"],
          "ties", int((counts[:out["stop"] + 1] == out["num_inliers"]).sum()),
          "global max", int(counts.max()), "at", int(counts.argmax()),
          "margin", out["min_margin"])
    assert (out["stop"], out["winner"], out["num_inliers"]) == (stop, winner, inliers)
    assert out["status"] == 0 and int(out["mask"].sum()) == inliers
    # no distance within 1e-9 of the threshold: fp64 rounding of a distance of
    # magnitude <= 40 is about 1e-14, so the counts and the mask of a correct
    # fp64 implementation are exactly these
    assert out["min_margin"] >= 1e-9


def test_cases_cover_their_situations(results):
    ties = {k: int((r["counts"][:r["stop"] + 1] == r["num_inliers"]).sum())
            for k, r in results.items()}
    assert ties[(90, 64, 8, 0.4)] == 12 and ties[(90, 400, 9, 0.5)] == 17
    assert ties[(33, 64, 11, 0.3)] == 21
    big = results[(2048, 400, 10, 0.6)]["counts"]  # the early exit hides a better hypothesis
    assert big.max() == 834 and big.argmax() == 10


def test_c_abi_validates_before_any_launch():
    import dpvo_amd

    lib = dpvo_amd.c_abi()
    wsb = lib.dpvo_ransac_umeyama_workspace_bytes
    wsb.restype = ctypes.c_size_t
    assert wsb(2048, 400) > wsb(33, 64) > 0
    f = lib.dpvo_ransac_umeyama
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                  ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    one = ctypes.c_void_p(1)  # never dereferenced: every call returns before a launch
    big = 1 << 20
    assert f(one, one, 2, 2, one, 4, 0.1, 100, one, one, one, one, big, None) == 1    # N = 2
    assert f(one, one, 33, 2, one, 0, 0.1, 100, one, one, one, one, big, None) == 1   # H = 0
    assert f(None, one, 33, 2, one, 4, 0.1, 100, one, one, one, one, big, None) == 1  # null src
    assert f(one, one, 33, 2, one, 4, 0.0, 100, one, one, one, one, big, None) == 1   # threshold
    assert f(one, one, 33, 2, one, 400, 0.1, 100, one, one, one, one, 16, None) == 4  # workspace
