"""The A-CORR edge order of the fused reprojection launch
(fastba.reproject(..., mem=, plan_window=)) at the sizes where its code
changes path.  Two properties are all A-CORR needs, and both must hold
exactly: the order is a permutation of 0..E-1, and the key (target frame,
16-pixel row band of the reprojected patch centre) is non-decreasing along it.

The key is recomputed here from the call's own outputs: frame = jj if
0 <= jj < min(mem, 64) else the last frame; band from the centre pixel's v of
the returned coords in float32, v >= 0 ? min(floor(v / 16), 15) : 0
(multiplying by 1/16 is exact, so this is the device's band bit for bit).

Sizes: E = 1, 63, 2047, 2048 (keys in registers), 4 * 512 + 1 (the first size
that recomputes keys in the second pass); target frames >= mem; all centres in
one band; negative v."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F, M, P = 12, 96, 3


def _graph(E, seed, y_lo=-60.0, y_hi=300.0, same_centre=False):
    rng = np.random.default_rng(seed)
    kk = rng.integers(0, F * M, E)
    ii, jj = kk // M, rng.integers(0, F, E)
    poses = np.zeros((F, 7), np.float32)
    poses[:, 6] = 1
    poses[:, :3] = rng.uniform(-0.05, 0.05, (F, 3))
    patches = np.ones((F * M, 3, P, P), np.float32)
    cx = rng.uniform(5, 300, F * M)
    cy = rng.uniform(y_lo, y_hi, F * M)
    if same_centre:
        cx[:], cy[:] = 100.0, 100.0
        poses[:, :3] = 0
    g = np.arange(P, dtype=np.float32) - P // 2
    patches[:, 0] = cx[:, None, None] + g[None, None, :]
    patches[:, 1] = cy[:, None, None] + g[None, :, None]
    patches[:, 2] = rng.uniform(0.5, 1.5, F * M)[:, None, None]
    return ii, jj, kk, poses, patches


CASES = {
    "E1": (dict(E=1, seed=0), F),
    "E63": (dict(E=63, seed=1), F),
    "E2047": (dict(E=2047, seed=2), F),
    "E2048": (dict(E=2048, seed=3), F),
    "E2049": (dict(E=4 * 512 + 1, seed=4), F),
    "frames_past_mem": (dict(E=1500, seed=5), 5),      # jj up to 11, mem = 5
    "one_band": (dict(E=1500, seed=6, same_centre=True), F),
    "negative_v": (dict(E=1500, seed=7, y_lo=-200.0, y_hi=-20.0), F),
}


@pytest.mark.parametrize("case", list(CASES))
def test_edge_order_is_a_sorted_permutation(gpu, case):
    from dpvo_amd import fastba

    kw, mem = CASES[case]
    ii, jj, kk, poses, patches = _graph(**kw)
    E = kk.size
    intr = np.tile(np.array([[80.0, 80.0, 80.0, 60.0]], np.float32), (F, 1))
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
           for x in (poses, patches, intr, ii.astype(np.int64), jj.astype(np.int64),
                     kk.astype(np.int64))]
    coords, order, ws = fastba.reproject(*dev, mem=mem, plan_window=(1, F))
    order = order.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(np.sort(order), np.arange(E))
    v = coords.cpu().numpy().reshape(E, 2, P, P)[:, 1, P // 2, P // 2].astype(np.float32)
    band = np.where(v >= 0, np.minimum(np.floor(v * np.float32(1.0 / 16.0)), np.float32(15)),
                    np.float32(0)).astype(np.int64)
    nf = min(max(mem, 1), 64)
    frame = np.where((jj >= 0) & (jj < nf), jj, nf - 1)
    key = frame * 16 + band
    if case == "one_band":
        assert np.unique(band).size == 1
    if case == "negative_v":
        assert (v < 0).all()
    if case == "frames_past_mem":
        assert (jj >= mem).any()
    assert (np.diff(key[order]) >= 0).all()
