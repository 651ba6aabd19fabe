"""CPU: the host logic of dpvo_amd.data_readers -- the sequence sampler on
hand-built graphs, the CSR of a given distance matrix against the reference's
np.where loop, read_disp, and discovery / pose permutation / index of the
TartanAir reader on a synthetic tree.  No GPU needed."""
import numpy as np
import pytest
import torch

import dataset_ref as ref
from dpvo_amd import data_readers as dr


def graph_of(rows, n=None):
    """{i: [(j, d), ..]} -> a host FrameGraph of n frames (d already times f)."""
    n = (max(rows) + 1) if n is None else n
    d = np.full((n, n), np.inf, np.float32)
    for i, row in rows.items():
        for j, v in row:
            d[i, j] = v
    return dr.FrameGraph.from_dense(d, 256)


def rng(seed=0):
    return np.random.default_rng(seed)


# ---- sample_sequence ---------------------------------------------------------------------
def test_forward_neighbour_is_preferred():
    # frame 0 sees 1 (too easy), 3 (in range) and 5 (too hard); 3 sees only 4 in range
    g = graph_of({0: [(0, 0.0), (1, 5.0), (3, 30.0), (5, 90.0)], 3: [(0, 30.0), (4, 20.0)],
                  4: [(2, 40.0)]}, n=8)
    assert dr.sample_sequence(g, 0, 3, 10.0, 75.0, True, rng()) == [0, 3, 4]
    # from 4 the only co-visible frame lies behind: ix + 1 is taken, not frame 2
    assert dr.sample_sequence(g, 3, 3, 10.0, 75.0, True, rng()) == [3, 4, 5]


def test_fall_through_to_next_frame():
    g = graph_of({0: [(0, 0.0)]}, n=4)
    assert dr.sample_sequence(g, 0, 4, sample=True, rng=rng()) == [0, 1, 2, 3]
    # the bounds are exclusive: a flow of exactly fmin or fmax does not count
    g = graph_of({0: [(2, 10.0), (3, 75.0)]}, n=4)
    assert dr.sample_sequence(g, 0, 2, 10.0, 75.0, True, rng()) == [0, 1]


def test_backward_choice_at_the_last_frame():
    g = graph_of({3: [(1, 30.0), (2, 5.0)], 1: [(0, 30.0)]}, n=4)
    # at the last frame nothing lies ahead and there is no ix + 1: frame 1 is drawn;
    # from 1, frame 0 (index zero does not count for np.count_nonzero) -> ix + 1
    assert dr.sample_sequence(g, 3, 3, 10.0, 75.0, True, rng()) == [3, 1, 2]
    # with nothing co-visible at the last frame the walk stays there
    assert dr.sample_sequence(graph_of({}, n=3), 2, 3, sample=True, rng=rng()) == [2, 2, 2]


def test_deterministic_walk_turns_at_both_ends():
    # budget d in (10, 75): every listed flow of 5 is inside it whatever d is drawn
    rows = {0: [(1, 5.0), (2, 6.0)], 2: [(3, 5.0), (0, 5.0)], 3: [(2, 5.0), (1, 6.0)],
            1: [(0, 5.0), (3, 5.0)]}
    g = graph_of(rows, n=4)
    # forward: the farthest frame ahead within the budget (0 -> 2 -> 3); at 3
    # nothing lies ahead and 3 + 1 is outside: the sign flips, 3 - 1 = 2; then
    # backward: from 2 the frames behind (0); at 0 nothing lies behind and
    # 0 - 1 < 0: the sign flips again, 0 + 1 = 1; forward from 1: frame 3
    assert dr.sample_sequence(g, 0, 7, 10.0, 75.0, False, rng()) == [0, 2, 3, 2, 0, 1, 3]


def test_deterministic_walk_respects_the_budget():
    g = graph_of({0: [(1, 5.0), (2, 9.0), (3, 200.0)]}, n=5)
    # 200 is over any budget in (10, 75): the farthest admissible frame is 2
    assert dr.sample_sequence(g, 0, 2, 10.0, 75.0, False, rng())[1] == 2
    # an empty row: ix + s
    assert dr.sample_sequence(g, 3, 2, 10.0, 75.0, False, rng()) == [3, 4]


def test_same_seed_same_list():
    n = 40
    r = np.random.default_rng(5)
    d = r.uniform(0, 120, (n, n)).astype(np.float32)
    g = dr.FrameGraph.from_dense(d, 256)
    for sample in (True, False):
        a = dr.sample_sequence(g, 3, 12, 10.0, 75.0, sample, rng(11))
        b = dr.sample_sequence(g, 3, 12, 10.0, 75.0, sample, rng(11))
        assert a == b and len(a) == 12 and all(0 <= i < n for i in a)
    walks = {tuple(dr.sample_sequence(g, 3, 12, 10.0, 75.0, True, rng(s))) for s in range(8)}
    assert len(walks) > 1


# ---- CSR ---------------------------------------------------------------------------------
def test_csr_matches_the_where_loop():
    r = np.random.default_rng(2)
    d = r.uniform(0, 500, (23, 23)).astype(np.float32)
    d[r.random((23, 23)) < 0.2] = np.inf
    d[5] = np.inf          # a row without neighbours
    d[7] = 1.0             # a row with all of them
    d[9, 3] = 256.0        # the bound is exclusive
    g = dr.FrameGraph.from_dense(d, 256)
    assert len(g) == 23 and g.rowptr.dtype == torch.int32 and g.col.dtype == torch.int32
    for i in range(23):
        j, = np.where(d[i] < 256)
        gj, gd = g.row(i)
        assert np.array_equal(gj, j) and np.array_equal(gd, d[i, j])
    assert len(g.row(5)[0]) == 0 and len(g.row(7)[0]) == 23 and 3 not in g.row(9)[0]


def test_graph_save_and_load(tmp_path):
    d = np.random.default_rng(3).uniform(0, 400, (9, 9)).astype(np.float32)
    g = dr.FrameGraph.from_dense(d, 256)
    g.save(tmp_path / "g.npz")
    h = dr.FrameGraph.load(tmp_path / "g.npz")
    for a, b in ((g.rowptr, h.rowptr), (g.col, h.col), (g.dist, h.dist)):
        assert a.dtype == b.dtype and torch.equal(a, b)


# ---- read_disp -----------------------------------------------------------------------------
@pytest.mark.parametrize("f", [4, 16])
def test_read_disp(f):
    depth = np.random.default_rng(4).uniform(0.5, 30.0, (64, 96)).astype(np.float32)
    depth[f // 2, f // 2] = 0.0       # a hole on the subsampled grid
    depth[0, 0] = 0.0                 # one off it: not seen
    keep = depth.copy()
    sub = depth[f // 2::f, f // 2::f].copy()
    want = sub.copy()
    want[sub < 0.01] = np.mean(sub)
    got = dr.read_disp(depth, f)
    assert got.shape == (64 // f, 96 // f)
    assert np.array_equal(got, 1.0 / want)
    assert np.array_equal(depth, keep)   # the caller's array is left alone


# ---- TartanAir on a synthetic tree -----------------------------------------------------------
@pytest.fixture()
def tree(tmp_path):
    return tmp_path, ref.write_tartan_tree(tmp_path)


def test_tartan_discovery_poses_and_index(tree):
    root, truth = tree
    (root / "envC" / "envC" / "Easy" / "P002" / "image_left").mkdir(parents=True)  # no frames: skipped
    db = dr.TartanAir(root, n_frames=3, crop_size=(24, 32), f=4, tail=2, device="cpu")
    assert sorted(db.scene_info) == sorted(truth)
    for scene, (imgs, deps, rows) in truth.items():
        info = db.scene_info[scene]
        assert len(info["images"]) == len(info["depths"]) == 8
        assert info["images"] == sorted(info["images"])
        want = rows[:, [1, 2, 0, 4, 5, 3, 6]].copy()
        want[:, :3] /= 5.0
        assert np.allclose(info["poses"], want, rtol=0, atol=1e-15)
        assert np.array_equal(np.stack(info["intrinsics"]), np.tile([320.0, 320.0, 320.0, 240.0], (8, 1)))
        assert np.array_equal(db.image_read(info["images"][3]), imgs[3])
        assert np.allclose(db.depth_read(info["depths"][3]), deps[3] / 5.0)
    # every frame but the last `tail` of every scene, scene by scene
    assert len(db) == 2 * 6
    assert db.dataset_index == [(s, i) for s in sorted(truth) for i in range(6)]
    db *= 3
    assert len(db) == 36


def test_tartan_test_split_and_default_tail(tree, tmp_path):
    root, truth = tree
    split = tmp_path / "split.txt"
    split.write_text("envB/envB/Hard/P001\nnot/there/Easy/P000\n")
    db = dr.TartanAir(root, f=4, tail=2, test_split=split, device="cpu")
    assert {s for s, _ in db.dataset_index} == {s for s in truth if "envA" in s}
    db = dr.TartanAir(root, f=4, tail=2, test_split=["envA/envA/Easy/P000"], device="cpu")
    assert {s for s, _ in db.dataset_index} == {s for s in truth if "envB" in s}
    assert len(dr.TartanAir(root, f=4, device="cpu")) == 0   # the reference's 65-frame tail


def test_golden_split_is_a_list_of_names():
    import os

    from conftest import GOLDEN

    names = dr.read_split(os.path.join(GOLDEN, "tartan_test_split.txt"))
    assert len(names) == 32 and len(set(names)) == 32
    assert all(len(n.split("/")) == 4 and n.split("/")[2] in ("Easy", "Hard") for n in names)


def test_depth_read_replaces_non_finite(tmp_path):
    d = np.array([[5.0, np.inf], [np.nan, 10.0]], np.float32)
    np.save(tmp_path / "d.npy", d)
    assert np.array_equal(dr.TartanAir.depth_read(tmp_path / "d.npy"), [[1.0, 1.0], [1.0, 2.0]])
