"""GPU: dpvo_amd.long_term.triangulate_tracks (csrc/triangulate.hip) against
the path it fuses, composed as long_term.py:108-136 composes it from ops this
tree already has: the mini patch graph, fastba.BA(..., t0=3, t1=3, M=-1,
iterations=6) (structure only; tests/test_ba_gpu.py test_structure_only checks
it against the oracle) and fastba.reproject.  Tolerances are that test's:
rtol 1e-4, atol 1e-5 on inverse depths (and on the points made from them)."""
import numpy as np
import pytest
import torch

import triangulate_ref as TR

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
MAX_RES, MAX_DEPTH = 2.0, 20.0


def _dev(S, gpu):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return dict(poses=t(S.poses), intrinsics=t(S.intrinsics), disps=t(S.disps), kps0=t(S.kps0),
                kps1=t(S.kps1), kps2=t(S.kps2), m10=t(S.m10), m12=t(S.m12))


def _existing_path(D, track):
    """long_term.py:93-136 on the tracks `track` (indices into kps1), with the
    ops of this tree -> (disp, points, residual) per track."""
    from dpvo_amd import fastba

    dev = D["poses"].device
    n = track.numel()
    kps0, kps1, kps2 = D["kps0"][D["m10"][track]], D["kps1"][track], D["kps2"][D["m12"][track]]
    kk = torch.arange(n, device=dev).repeat(2)
    ii = torch.ones(2 * n, device=dev, dtype=torch.long)
    jj = torch.zeros(2 * n, device=dev, dtype=torch.long)
    jj[n:] = 2
    true_disp = D["disps"].median()
    patches = torch.cat([kps1, true_disp.expand(n, 1)], dim=-1)  # [n, 3] (u, v, d)
    patches = patches.view(n, 3, 1, 1).expand(n, 3, 3, 3).contiguous()
    target = torch.cat([kps0, kps2])[None].contiguous()  # [1, 2n, 2]
    weight = torch.ones_like(target)
    poses, intrinsics = D["poses"].clone(), D["intrinsics"].clone()
    lmbda = torch.as_tensor([1e-3], device=dev)
    fastba.BA(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, 3, 3, M=-1,
              iterations=6)
    assert torch.equal(poses, D["poses"])
    coords = fastba.reproject(poses, patches, intrinsics, ii, jj, kk)[0, :, :, 1, 1]
    residual = (coords - target[0]).norm(dim=-1)
    residual = torch.maximum(residual[:n], residual[n:])
    K = intrinsics[1]
    d = patches[:, 2, 1, 1]
    pts = torch.stack([(kps1[:, 0] - K[2]) / K[0], (kps1[:, 1] - K[3]) / K[1],
                       torch.ones_like(d)], 1) / d[:, None]
    return d, pts, residual


@pytest.mark.parametrize("N1,M", [(1, 8), (5, 7), (64, 8), (300, 7)])
def test_against_existing_path(gpu, N1, M):
    from dpvo_amd.long_term import triangulate_tracks

    S = TR.scene(N1, M)
    D = _dev(S, gpu)
    out = triangulate_tracks(**D)
    assert out.points.shape == (N1, 3) and out.disp.shape == (N1,) and out.keep.dtype == torch.bool
    assert out.sel.dtype == torch.int64 and out.count.dtype == torch.int32
    m10, m12 = D["m10"], D["m12"]
    is_track = (m10 >= 0) & (m10 < S.kps0.shape[0]) & (m12 >= 0) & (m12 < S.kps2.shape[0])
    track = torch.nonzero(is_track)[:, 0]
    d, pts, res = _existing_path(D, track)

    np.testing.assert_allclose(out.disp[track].cpu().numpy(), d.cpu().numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.points[track].cpu().numpy(), pts.cpu().numpy(), rtol=RTOL,
                               atol=ATOL)
    assert not out.keep[~is_track].any()
    assert (out.points[~is_track] == 0).all() and (out.disp[~is_track] == 0).all()
    keep_ref = (res < MAX_RES) & (pts[:, 2] < MAX_DEPTH)
    near = ((res - MAX_RES).abs() <= RTOL * MAX_RES + ATOL) | \
           ((pts[:, 2] - MAX_DEPTH).abs() <= RTOL * MAX_DEPTH + ATOL)
    excused = int(near.sum())
    print(f"N1 {N1}: tracks {track.numel()}, kept {int(keep_ref.sum())}, excused {excused}")
    assert excused <= 0.02 * track.numel() and (N1 > 64 or excused == 0)
    assert torch.equal(out.keep[track][~near], keep_ref[~near])

    # the scene's special keypoints (triangulate_ref.scene)
    keep = out.keep.cpu().numpy()
    assert keep[0]
    if N1 >= 5:
        assert not is_track[1] and not is_track[2]
        r3, r4 = res[(track == 3).nonzero()[0, 0]], res[(track == 4).nonzero()[0, 0]]
        assert float(r3) > 10 and not keep[3]  # the 40 px observation: residual gate
        assert float(r4) < 0.5 and float(out.points[4, 2]) > 20 and not keep[4]  # depth 30
    if N1 >= 64:
        assert not is_track[5] and not is_track[7]
        assert float(out.disp[6]) == np.float32(1e-4) and not keep[6]  # clamp of the retraction
        noisy = keep[32::4]
        assert noisy.any() and not noisy.all()

    # sel: the kept indices ascending, then -1; count
    kept = np.nonzero(keep)[0]
    sel, count = out.sel.cpu().numpy(), int(out.count)
    assert count == len(kept)
    np.testing.assert_array_equal(sel[:count], kept)
    assert (sel[count:] == -1).all()

    # the fp64 restatement agrees too (fp32 edge math against fp64: looser)
    ref = TR.triangulate_ref(S.poses, S.intrinsics, S.disps, S.kps0, S.kps1, S.kps2, S.m10, S.m12)
    t = track.cpu().numpy()
    np.testing.assert_allclose(out.disp.cpu().numpy()[t], ref.disp[t], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("M", [1, 2, 7, 8, 80, 1024])
def test_lower_median_start(gpu, M):
    """iterations=0 returns the start value: torch.median of the M depths (the
    lower of the two middle values for an even M), through a strided view."""
    from dpvo_amd.long_term import triangulate_tracks

    S = TR.scene(5, 8)
    D = _dev(S, gpu)
    g = torch.Generator().manual_seed(M)
    patches = torch.rand(M, 3, 3, 3, generator=g).to(gpu)
    if M >= 8:
        patches[3, 2, 1, 1] = patches[5, 2, 1, 1]  # a tie
    D["disps"] = patches[:, 2, 1, 1]
    out = triangulate_tracks(**D, iterations=0)
    is_track = (D["m10"] >= 0) & (D["m12"] >= 0)
    want = D["disps"].median()
    assert (out.disp[is_track] == want).all() and is_track.sum() == 3
    if M == 2:
        assert want == D["disps"].min()


def test_iterations_and_gates_are_arguments(gpu):
    from dpvo_amd.long_term import triangulate_tracks

    S = TR.scene(64, 8)
    D = _dev(S, gpu)
    base = triangulate_tracks(**D)
    wide = triangulate_tracks(**D, max_depth=40.0, max_residual=50.0)
    assert torch.equal(base.disp, wide.disp)
    assert wide.keep[3] and wide.keep[4] and not base.keep[3] and not base.keep[4]
    assert int(wide.count) == int(wide.keep.sum()) > int(base.count)
    again = triangulate_tracks(**D)
    for x, y in zip(base, again):
        assert torch.equal(x, y)
