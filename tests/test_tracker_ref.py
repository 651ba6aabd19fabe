"""CPU: the restatement in tests/tracker_ref.py against the reference's own
expressions (dpvo/dpvo.py:917, 937-938 and 838-903)."""
import numpy as np
import pytest
import torch

import tracker_ref as T


def test_colour_chain_is_the_reference_expression_and_not_the_identity():
    p = torch.arange(256, dtype=torch.uint8)
    image = 2 * (p[None, None] / 255.0) - 0.5  # dpvo.py:917
    ref = ((image[0, 0] + 0.5) * (255.0 / 2)).to(torch.uint8)  # dpvo.py:937-938
    got = T.color_chain(p)
    assert torch.equal(got, ref)
    diff = (got != p).nonzero().reshape(-1)
    assert diff.numel() == 31
    assert torch.equal(got[diff].int(), p[diff].int() - 1)
    assert diff[:12].tolist() == list(range(1, 13))


def _flatmeshgrid(a, b):
    g = torch.meshgrid(a, b, indexing="ij")
    return g[0].reshape(-1), g[1].reshape(-1)


@pytest.mark.parametrize("r", [3, 12])
def test_edge_lists_equal_flatmeshgrid(r):
    M = 4
    for n in range(1, 15):
        # dpvo.py:867-872
        kf, jf = _flatmeshgrid(torch.arange(M * max(n - r, 0), M * max(n - 1, 0)),
                               torch.arange(n - 1, n))
        # dpvo.py:899-903
        kb, jb = _flatmeshgrid(torch.arange(M * max(n - 1, 0), M * max(n, 0)),
                               torch.arange(max(n - r, 0), n))
        assert T.edges_forw(n, M, r) == (kf.tolist(), jf.tolist())
        assert T.edges_back(n, M, r) == (kb.tolist(), jb.tolist())


def test_frame_sample_restatement_against_a_loop():
    g = torch.Generator().manual_seed(0)
    h, w, P = 6, 9, 3
    fmap, imap = torch.randn(4, h, w, generator=g), torch.randn(5, h, w, generator=g)
    image = T.normalise(torch.randint(0, 256, (3, 4 * h, 4 * w), generator=g, dtype=torch.uint8))
    coords = torch.tensor([[1.0, 1.0], [7.0, 4.0], [3.0, 2.0]])
    gm, im, pt, clr = T.frame_sample(fmap, imap, image, coords, P)
    for m, (x, y) in enumerate(coords.long().tolist()):
        assert torch.equal(gm[m], fmap[:, y - 1:y + 2, x - 1:x + 2])
        assert torch.equal(im[m], imap[:, y, x])
        assert pt[m, 0, 1].tolist() == [x - 1, x, x + 1] and pt[m, 1, :, 1].tolist() == [y - 1, y, y + 1]
        assert (pt[m, 2] == 1).all()
        px = image[:, 4 * y + 2, 4 * x + 2]
        assert torch.equal(clr[m], ((px[[2, 1, 0]] + 0.5) * 127.5).to(torch.uint8))


def test_map_points_restatement_round_trip():
    rng = np.random.default_rng(0)
    q = rng.normal(size=(3, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.concatenate([rng.normal(size=(3, 3)), q], 1)
    patches = rng.uniform(0.5, 2.0, size=(6, 3, 3, 3))
    intr = np.tile([50.0, 60.0, 20.0, 15.0], (3, 1))
    ix = np.repeat(np.arange(3), 2)
    X = T.map_points(poses, patches, intr, ix, 6)
    # the world point mapped back by the pose projects onto the patch centre at depth 1 / d
    R = T.quat_to_matrix(poses[ix, 3:])
    Y = np.einsum("kij,kj->ki", R, X) + poses[ix, :3]
    np.testing.assert_allclose(Y[:, 2], 1.0 / patches[:, 2, 1, 1], rtol=1e-12)
    np.testing.assert_allclose(50.0 * Y[:, 0] / Y[:, 2] + 20.0, patches[:, 0, 1, 1], rtol=1e-12)
    np.testing.assert_allclose(60.0 * Y[:, 1] / Y[:, 2] + 15.0, patches[:, 1, 1, 1], rtol=1e-12)


def test_bookkeeping_without_drops_matches_the_window_rule():
    M, r, rw = 2, 3, 5
    b = T.Bookkeeping(M, r, rw, 4)
    for _ in range(20):
        b.frame()
    assert (b.n, b.m, b.counter) == (20, 40, 20) and b.updates == 12 + 12
    ii, jj, kk = b.edge_arrays()
    assert ii.min() == b.n - rw and (ii == kk // M).all()
    assert [b.tstamps[i] for i in range(b.n)] == list(range(20))
    # a rejected frame before initialisation leaves n and logs (t, t - 1)
    b = T.Bookkeeping(M, r, rw, 4)
    b.frame()
    b.frame(probe_ok=False)
    b.frame(probe_ok=False)
    assert (b.n, b.counter, b.delta) == (1, 3, [(1, 0), (2, 1)])
