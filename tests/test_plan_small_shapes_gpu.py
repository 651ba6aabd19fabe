"""The BA plan (edges grouped by patch) at the sizes where its code changes
path, through fastba.plan and through the fused reprojection launch
(fastba.reproject(..., plan_window=...)), against a numpy grouping: a stable
argsort of kk, the first position and id of every patch, and the free-pose
masks from ii / jj against the window.  Exact equality of epos, poff, pkk,
pmask, nuniq, fmin, status and (sharded plans) the summed block work.

Sizes: E = 1; 512 / 513 (one shard, then two); 2048 / 2049 (the last size of
the copy unrolled 4 deep, then the first of the long one); 1000 (no multiple
of 64).  At E = 2048: one patch, one patch per edge, a kk range with gaps so
wide that shards own no edge, duplicated (ii, jj, kk) triples, every pose
fixed.  The shard count is a function of E alone (not tunable)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = 12  # poses


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    m = dpvo_amd.load_extension("cuda_ba")
    m.check_status(torch.zeros(1, device=gpu))
    return m


def _grouping(ii, jj, kk, t0, t1):
    order = np.argsort(kk, kind="stable")
    uk, first = np.unique(kk[order], return_index=True)
    poff = np.append(first, kk.size)
    bits = np.zeros(kk.size, np.uint32)
    for x in (ii, jj):
        free = (x >= t0) & (x < t1)
        bits |= np.where(free, np.left_shift(1, np.clip(x - t0, 0, 31)), 0).astype(np.uint32)
    pmask = np.array([np.bitwise_or.reduce(bits[order[poff[u]:poff[u + 1]]])
                      for u in range(uk.size)], np.uint32)
    return order.astype(np.int32), poff.astype(np.int32), pmask, uk.astype(np.int32)


def _block_work(ref, N):
    want = np.zeros(136, np.int64)
    poff, pmask = ref[1], ref[2]
    for u in range(pmask.size):
        c, m = int(poff[u + 1] - poff[u]), int(pmask[u])
        bits = [x for x in range(N) if (m >> x) & 1]
        for x in bits:
            for y in bits:
                if y <= x:
                    want[x * (x + 1) // 2 + y] += c
    return want


def _arrays(cb, ws, E, t0, t1):
    off = cb.plan_offsets(E, t0, t1)
    b = ws.cpu().numpy()

    def arr(k, n, dt):
        return np.frombuffer(b[off[k]:off[k] + 4 * n].tobytes(), dt)

    meta = arr(4, 64 + 16 * 136, np.int32)
    nuniq = int(meta[0])
    return (arr(0, E, np.int32), arr(1, nuniq + 1, np.int32), arr(2, nuniq, np.uint32),
            arr(3, nuniq, np.int32), nuniq, meta)


def _random(E, nk, M, seed):
    rng = np.random.default_rng(seed)
    base = np.sort(rng.choice(F * M, nk, replace=False))
    kk = rng.permutation(np.concatenate([base, base[rng.integers(0, nk, E - nk)]]))
    return kk // M, rng.integers(0, F, E), kk, M, (1, F)


def _one_patch(E, M):
    rng = np.random.default_rng(20)
    kk = np.full(E, 5 * M + 7)
    return kk // M, rng.integers(0, F, E), kk, M, (1, F)


def _own_patch(E, M):
    rng = np.random.default_rng(21)
    kk = rng.permutation(np.arange(100, 100 + E))
    return kk // M, rng.integers(0, F, E), kk, M, (1, F)


def _gaps(E, M):
    """Two clusters of 40 patch ids at the ends of a range of 3000: the
    middle shards of the range own no edge."""
    rng = np.random.default_rng(22)
    kk = np.where(rng.integers(0, 2, E) == 0, rng.integers(0, 40, E), rng.integers(2960, 3000, E))
    return kk // M, rng.integers(0, F, E), kk, M, (1, F)


def _duplicates(E, M):
    rng = np.random.default_rng(23)
    kk = np.tile(rng.choice(F * M, 64, replace=False), E // 64)
    jj = np.tile(rng.integers(0, F, 64), E // 64)
    return kk // M, jj, kk, M, (1, F)


def _all_fixed(E, M):
    rng = np.random.default_rng(24)
    kk = rng.integers(0, 10 * M, E)  # ii, jj < 10: outside the window [10, 12)
    return kk // M, rng.integers(0, 10, E), kk, M, (10, F)


CASES = {
    "E1": lambda: _random(1, 1, 96, 0),
    "E512": lambda: _random(512, 200, 96, 1),
    "E513": lambda: _random(513, 200, 96, 2),
    "E1000": lambda: _random(1000, 300, 96, 3),
    "E2048": lambda: _random(2048, 700, 96, 4),
    "E2049": lambda: _random(2049, 700, 96, 5),
    "E2048_one_patch": lambda: _one_patch(2048, 96),
    "E2048_own_patch": lambda: _own_patch(2048, 256),
    "E2048_gaps": lambda: _gaps(2048, 256),
    "E2048_duplicates": lambda: _duplicates(2048, 96),
    "E2048_all_fixed": lambda: _all_fixed(2048, 96),
}


def _check(got, ref, fmin, N, sharded):
    epos, poff, pmask, pkk, nuniq, meta = got
    assert nuniq == ref[3].size
    assert int(meta[1]) == fmin and int(meta[2]) == 0
    np.testing.assert_array_equal(pkk, ref[3])
    np.testing.assert_array_equal(poff, ref[1])
    np.testing.assert_array_equal(epos, ref[0])
    np.testing.assert_array_equal(pmask, ref[2])
    nsh = int(meta[3])
    if sharded:
        assert nsh > 1  # these graphs fit the sharded plan: it must not have fallen back
    if nsh:
        work = meta[64:64 + 16 * 136].reshape(136, 16)[:, :nsh].sum(1)
        nb = N * (N + 1) // 2
        np.testing.assert_array_equal(work[:nb], _block_work(ref, N)[:nb])


@pytest.mark.parametrize("case", list(CASES))
def test_plan_matches_numpy_grouping(cb, gpu, case):
    from dpvo_amd import fastba

    ii, jj, kk, M, (t0, t1) = CASES[case]()
    ii, jj, kk = (np.ascontiguousarray(x, np.int64) for x in (ii, jj, kk))
    E = kk.size
    ref = _grouping(ii, jj, kk, t0, t1)
    both = np.concatenate([ii, jj])
    fixed = both[(both < t0) | (both >= t1)]
    fmin = int(np.clip(fixed.min(), 0, F - 1)) if fixed.size else 2 ** 31 - 1
    if case == "E2048_all_fixed":
        assert not ref[2].any()
    D = [torch.from_numpy(x).to(gpu) for x in (ii, jj, kk)]
    for rep in range(2):
        ws = fastba.plan(*D, t0, t1, F * M, F)
        assert ws is not None
        _check(_arrays(cb, ws, E, t0, t1), ref, fmin, t1 - t0, E > 512)
    poses = torch.zeros(F, 7, device=gpu)
    poses[:, 6] = 1
    patches = torch.ones(F * M, 3, 3, 3, device=gpu)
    intr = torch.tensor([[80.0, 80.0, 80.0, 60.0]], device=gpu).repeat(F, 1)
    _, _, ws = fastba.reproject(poses, patches, intr, *D, mem=F, plan_window=(t0, t1))
    _check(_arrays(cb, ws, E, t0, t1), ref, fmin, t1 - t0, E > 512)
    assert cb.check_status(poses) == 0
