"""GPU: the TartanAir reader end to end on the synthetic tree of
tests/dataset_ref.py -- two scenes of 8 frames at 32 x 48, f = 4."""
import numpy as np
import pytest
import torch

import dataset_ref as ref

pytestmark = pytest.mark.gpu

KW = dict(n_frames=4, crop_size=(24, 32), fmin=0.0, fmax=1e9, f=4, tail=2)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("tartan")
    return root, ref.write_tartan_tree(root)


def test_item_shapes_and_dtypes(gpu, tree):
    from dpvo_amd.data_readers import TartanAir

    root, _ = tree
    db = TartanAir(root, seed=0, **KW)
    images, poses, disps, intrinsics = db[0]
    for t, shape in ((images, (1, 4, 3, 24, 32)), (poses, (1, 4, 7)), (disps, (1, 4, 24, 32)),
                     (intrinsics, (1, 4, 4))):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
        assert torch.isfinite(t).all()
    # the depth normalisation: 0.7 quantile(disps, 0.98) is 1 afterwards
    assert abs(float(torch.quantile(disps.cpu().reshape(-1), 0.98)) - 1 / 0.7) < 1e-4


def test_item_without_augmentation_is_the_files(gpu, tree):
    from dpvo_amd.data_readers import TartanAir, normalize_depth

    root, truth = tree
    db = TartanAir(root, aug=False, sample=False, seed=0, **KW)
    scene, ix = db.dataset_index[7]
    imgs, deps, rows = truth[scene]
    inds = [ix]
    images, poses, disps, intrinsics = db[7]
    # whichever frames the walk took, the item holds those files: find them by the image
    for n in range(4):
        got = images[0, n].cpu().permute(1, 2, 0).numpy()[..., ::-1]      # BGR planes -> RGB
        match = [i for i in range(8) if np.array_equal(got, imgs[i].astype(np.float32))]
        assert len(match) == 1
        inds.append(match[0])
    assert inds[1] == ix
    sel = inds[1:]
    d = torch.from_numpy(1.0 / (deps[sel] / 5.0)).to(gpu)
    want_p = rows[sel][:, [1, 2, 0, 4, 5, 3, 6]].copy()
    want_p[:, :3] /= 5.0
    wd, wp = normalize_depth(d, torch.from_numpy(want_p.astype(np.float32)).to(gpu))
    assert torch.allclose(disps[0], wd, rtol=1e-6, atol=0) and torch.allclose(poses[0], wp, rtol=1e-6)
    assert torch.equal(intrinsics[0].cpu(), torch.tensor([[320.0, 320.0, 320.0, 240.0]]).repeat(4, 1))


def test_fixed_rng_gives_identical_output(gpu, tree):
    from dpvo_amd.data_readers import TartanAir

    root, _ = tree
    db = TartanAir(root, seed=0, **KW)
    for index in (0, 5, 11):
        a = db.__getitem__(index, rng=np.random.default_rng(42))
        b = db.__getitem__(index, rng=np.random.default_rng(42))
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    db2 = TartanAir(root, seed=9, **KW)
    db3 = TartanAir(root, seed=9, **KW)
    assert all(torch.equal(x, y) for x, y in zip(db2[3], db3[3]))


def test_cached_graph_reloads_equal(gpu, tree, tmp_path):
    from dpvo_amd.data_readers import FrameGraph, TartanAir, build_frame_graph, read_disp

    root, truth = tree
    db = TartanAir(root, cache=tmp_path / "cache", seed=0, **KW)
    scene = sorted(truth)[1]
    g = db.scene_graph(scene)
    files = list((tmp_path / "cache").glob("*.npz"))
    assert len(files) == 1 and len(g) == 8
    h = FrameGraph.load(files[0])
    for a, b in ((g.rowptr, h.rowptr), (g.col, h.col), (g.dist, h.dist)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # a second reader takes it from the cache, without the device
    db2 = TartanAir(root, cache=tmp_path / "cache", seed=0, device="cpu", **KW)
    k = db2.scene_graph(scene)
    assert torch.equal(k.col, g.col) and torch.equal(k.dist, g.dist)
    # and it is the graph of the files: read_disp, intrinsics / f
    imgs, deps, rows = truth[scene]
    disps = np.stack([read_disp(d / 5.0, 4) for d in deps])
    poses = rows[:, [1, 2, 0, 4, 5, 3, 6]].copy()
    poses[:, :3] /= 5.0
    to = dict(device=gpu, dtype=torch.float32)
    want = build_frame_graph(torch.as_tensor(poses, **to), torch.as_tensor(disps, **to),
                             torch.as_tensor(np.tile([80.0, 80.0, 80.0, 60.0], (8, 1)), **to), f=4).cpu()
    assert torch.equal(want.rowptr, g.rowptr) and torch.equal(want.dist, g.dist)
    assert len(g.row(0)[0]) >= 1     # at least itself
