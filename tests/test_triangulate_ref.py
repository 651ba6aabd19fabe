"""CPU: the numpy restatement of triangulate_tracks (triangulate_ref.py) on
its synthetic triplet -- it recovers the depths the scene was built from and
gates what the scene says it gates."""
import numpy as np
import pytest

import triangulate_ref as TR


def _run(S, **kw):
    return TR.triangulate_ref(S.poses, S.intrinsics, S.disps, S.kps0, S.kps1, S.kps2, S.m10, S.m12,
                              **kw)


@pytest.mark.parametrize("N1,M", [(1, 8), (5, 7), (64, 8), (300, 7)])
def test_scene_and_restatement(N1, M):
    S = TR.scene(N1, M)
    out = _run(S)
    assert out.track[0] and out.keep[0]
    plain = out.track.copy()
    plain[[k for k in (3, 4, 6) if k < N1]] = False
    if N1 >= 64:
        plain[32::4] = False
    # 0.05 px of noise over a 0.1 baseline at fx = 320: a few 1e-3 in inverse depth
    np.testing.assert_allclose(out.disp[plain], 1.0 / S.depth[plain], atol=5e-3)
    np.testing.assert_allclose(out.points[plain, 2], S.depth[plain], rtol=2e-2)
    assert out.keep[plain].all() and (out.residual[plain] < 0.5).all()
    if N1 >= 5:
        assert not out.track[1] and not out.track[2]
        assert out.track[3] and out.residual[3] > 10 and not out.keep[3]
        assert out.track[4] and out.residual[4] < 0.5 and out.points[4, 2] > 20 and not out.keep[4]
    if N1 >= 64:
        assert not out.track[5] and not out.track[7]
        assert out.disp[6] == 1e-4 and not out.keep[6]
        noisy = out.residual[32::4]
        assert (noisy < 2).any() and (noisy >= 2).any()
    kept = np.nonzero(out.keep)[0]
    assert out.count == len(kept) and (out.sel[:out.count] == kept).all()
    assert (out.sel[out.count:] == -1).all()
    assert (out.points[~out.track] == 0).all() and (out.disp[~out.track] == 0).all()


def test_lower_median_and_no_iterations():
    assert TR.lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0  # not 2.5
    assert TR.lower_median([3.0, 1.0, 2.0]) == 2.0
    assert TR.lower_median([5.0]) == 5.0
    for M in (7, 8):
        S = TR.scene(5, M)
        out = _run(S, iterations=0)
        assert (out.disp[out.track] == np.sort(S.disps)[(M - 1) // 2]).all()
