"""GPU: frame_distance_matrix and build_frame_graph (csrc/dataset.hip) against the
fp64 restatement of tests/dataset_ref.py.

Kernel and restatement both compute in fp64 from the same fp32 inputs; what
separates them is the final rounding to fp32 and the order of the sums, so the
tolerance is rtol 1e-6, atol 1e-6: a few fp32 ulps of margin.  An entry may be
left out of the comparison only when, in the restatement, some point of the
pair lies within 1e-6 of the Z = 0.2 validity bound (at most 1 % of a case;
the seeds are chosen so that no entry is)."""
import numpy as np
import pytest
import torch

import dataset_ref as ref

pytestmark = pytest.mark.gpu

# (N, h, w, seed, special frames): under one wave; 63 points, odd; two waves and a
# remainder; more frames than one tile of 64
CASES = {
    "n5_6x8": (5, 6, 8, 1, ["base", "above", "below", "turn", "clamp"]),
    "n5_7x9": (5, 7, 9, 2, ["base", "rot", "trans", "above", "below"]),
    "n9_10x13": (9, 10, 13, 3, None),
    "n70_6x8": (70, 6, 8, 4, None),
}
_cache = {}


def case(name):
    if name not in _cache:
        N, h, w, seed, pick = CASES[name]
        poses, disps, K, roles = ref.make_scene(N, h, w, seed, pick)
        _cache[name] = (poses, disps, K, roles) + ref.flow_distance(poses, disps, K)
    return _cache[name]


def device_D(gpu, name):
    from dpvo_amd import data_readers as dr

    poses, disps, K = (torch.from_numpy(a).to(gpu) for a in case(name)[:3])
    return dr.frame_distance_matrix(poses, disps, K), (poses, disps, K)


@pytest.mark.parametrize("name", list(CASES))
def test_scene_holds_what_it_should(name):
    """On the restatement alone: the special pairs are what they claim to be."""
    poses, disps, K, roles, D, k, near = case(name)
    N, h, w = disps.shape
    ka, kb = ref.share_counts(h * w)
    b = roles["base"]
    assert not near.any()                                  # nothing to exclude
    assert k[b, roles["above"]] == ka and np.isfinite(D[b, roles["above"]])
    assert k[b, roles["below"]] == kb and np.isinf(D[b, roles["below"]])
    if "turn" in roles:
        assert k[b, roles["turn"]] == 0 and np.isinf(D[b, roles["turn"]])
    if "clamp" in roles:
        assert D[b, roles["clamp"]] == 100.0
    for r in ("rot", "trans"):
        if r in roles:
            assert 0.01 < D[b, roles[r]] < 100.0
    assert len({tuple(row) for row in K}) == N             # per-frame intrinsics
    assert np.all(np.diag(D) < 1e-6)


@pytest.mark.parametrize("name", list(CASES))
def test_distance_matrix(gpu, name):
    poses, disps, K, roles, D, k, near = case(name)
    assert near.mean() <= 0.01
    got, _ = device_D(gpu, name)
    again, _ = device_D(gpu, name)
    assert got.dtype == torch.float32 and got.shape == (len(poses),) * 2
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))        # run to run
    assert torch.equal(got.view(torch.int32), got.T.contiguous().view(torch.int32))  # symmetric
    got = got.cpu().numpy()
    ok = ~near
    assert np.array_equal(np.isinf(got)[ok], np.isinf(D)[ok])
    fin = ok & np.isfinite(D)
    err = np.abs(got[fin].astype(np.float64) - D[fin])
    print(name, "max abs err", err.max(), "finite", fin.sum(), "inf", np.isinf(D).sum())
    assert np.all(err <= 1e-6 + 1e-6 * np.abs(D[fin]))


@pytest.mark.parametrize("name", ["n5_6x8", "n70_6x8"])
@pytest.mark.parametrize("f,max_flow", [(16, 256), (4, 30)])
def test_build_frame_graph(gpu, name, f, max_flow):
    from dpvo_amd import data_readers as dr

    D, (poses, disps, K) = device_D(gpu, name)
    g = dr.build_frame_graph(poses, disps, K, f=f, max_flow=max_flow)
    assert g.rowptr.is_cuda and g.rowptr.dtype == torch.int32 and g.col.dtype == torch.int32
    d = np.float32(f) * D.cpu().numpy()
    want = dr.FrameGraph.from_dense(d, max_flow)
    g = g.cpu()
    assert torch.equal(g.rowptr, want.rowptr) and torch.equal(g.col, want.col)
    assert torch.equal(g.dist.view(torch.int32), want.dist.view(torch.int32))
    j, dist = g.row(0)
    assert np.array_equal(j, np.where(d[0] < max_flow)[0]) and np.array_equal(dist, d[0, j])


@pytest.mark.parametrize("N", [7, 300, 1100])   # one chunk; several of 256; a scan past 1024
def test_frame_graph_rows(gpu, N):
    """The CSR kernels on a given matrix: a row without neighbours, a row with all N."""
    import dpvo_amd
    from dpvo_amd import data_readers as dr

    ext = dpvo_amd.load_extension("cuda_ba")
    r = np.random.default_rng(N)
    D = r.uniform(0, 40, (N, N)).astype(np.float32)
    D[r.random((N, N)) < 0.3] = np.inf
    D[2] = np.inf
    D[N - 1] = np.inf
    D[4] = 0.5
    D[5, 1] = 16.0     # 16 * 16 = 256: the bound is exclusive
    rowptr, col, dist = (t.cpu() for t in ext.frame_graph(torch.from_numpy(D).to(gpu), 16.0, 256.0))
    want = dr.FrameGraph.from_dense(np.float32(16) * D, 256)
    assert torch.equal(rowptr, want.rowptr) and torch.equal(col, want.col)
    assert torch.equal(dist.view(torch.int32), want.dist.view(torch.int32))
    assert rowptr[3] == rowptr[2] and rowptr[N] == rowptr[N - 1] and rowptr[5] - rowptr[4] == N
    # nothing below the bound at all: empty outputs
    rowptr, col, dist = ext.frame_graph(torch.full((N, N), np.inf, device=gpu), 16.0, 256.0)
    assert int(rowptr.abs().sum()) == 0 and col.numel() == 0 and dist.numel() == 0
