"""CPU checks of the large-graph BA case table (gba_cases.py): every case has
the band structure its row claims, the table as a whole reaches every solver
branch it is there for, the structure restatement agrees with the sparsity of
the oracle's dense S, and the parity cases stay clear of the discontinuous
depth clamps (which have their own tests, test_ba_gates_gpu.py).  No GPU.

Run with -s to list, per case: (nI, nB, g, nsb), the largest pose set,
cond(S), the oracle status and the inverse-depth range after 1 and 2
iterations."""
import numpy as np
import pytest

import gba_cases as gc
import oracle

_cache = {}


def _oracle(name, iters):
    """oracle.ba(..., diagnostics=True) of the case (computed once; read-only)."""
    if (name, iters) not in _cache:
        G, t0 = gc.graph(name), gc.CASES[name]["t0"]
        _cache[name, iters] = oracle.ba(
            G.poses.numpy(), G.patches.numpy(), G.intrinsics.numpy(), G.target.numpy(),
            G.weight.numpy(), 1e-4, G.ii.numpy(), G.jj.numpy(), G.kk.numpy(), t0, G.F, iters,
            diagnostics=True)
    return _cache[name, iters]


@pytest.mark.parametrize("name", list(gc.CASES))
def test_case_has_the_structure_its_row_claims(name):
    c, st = gc.CASES[name], gc.case_structure(name)
    G = gc.graph(name)
    assert (st["nI"], st["nB"], st["g"], st["nsb"]) == c["expect"]
    assert st["nI"] + st["nB"] == G.F - c["t0"]
    assert st["nuniq"] == len(np.unique(G.kk.numpy()))
    assert G.F - c["t0"] <= 150 and G.E < 1000  # a few seconds on the GPU at most
    if c["kind"] == "parity":
        assert st["maxset"] <= gc.MAX_SET and st["nB"] <= gc.MAX_BORDER
    print(f"\n{name}: E={G.E} (nI, nB, g, nsb)={c['expect']} largest set={st['maxset']} "
          f"nblk={st['nblk']} nitems={st['nitems']}")


def test_table_reaches_every_branch():
    seen = {}
    for name in gc.PARITY:
        for b in gc.branches(gc.case_structure(name)):
            seen.setdefault(b, []).append(name)
    missing = gc.REQUIRED_BRANCHES - set(seen)
    assert not missing, sorted(missing)
    # (g, nsb, nB class) of the parity cases, as the issue lists them
    cov = {gc.CASES[n]["expect"] for n in gc.PARITY}
    assert {g for _, _, g, _ in cov} >= {1, 2, 5, 13, 14, 16}
    assert {s for _, _, _, s in cov} >= {1, 2, 3, 4, 5, 6, 7, 9} and max(s for *_, s in cov) > gc.BP
    assert {b for _, b, _, _ in cov} >= {0, 1, 16, 17, 64}
    assert any(nI % g for nI, _, g, _ in cov if g == 16)  # padded last superblock at m = 96
    assert gc.two_fit(13) and not gc.two_fit(14)
    # both staging forms of both two-product kernels, either side of the switch
    for g, form in ((13, "two_fit"), (14, "sequential"), (16, "sequential")):
        for kern in ("cr_b_both:", "cr_back_r:"):
            assert any(gc.CASES[n]["expect"][2] == g for n in seen[kern + form]), (g, kern)
    a, b = gc.graph("nB17"), gc.graph("chain_like_nB17")  # same workspace size
    assert (a.E, a.F) == (b.E, b.F)
    # the status cases sit one step past their limit, next to a clean neighbour
    s25, s24 = gc.case_structure("set25"), gc.case_structure("set24")
    assert (s25["maxset"], s24["maxset"]) == (gc.MAX_SET + 1, gc.MAX_SET)
    assert gc.branches(s25) >= {"status_set"} and "status_set" not in gc.branches(s24)
    assert gc.case_structure("nB65")["nB"] == gc.MAX_BORDER + 1
    assert gc.branches(gc.case_structure("nB65")) == {"status_border"}
    assert gc.CASES["set24"]["kind"] == gc.CASES["nB64"]["kind"] == "parity"
    # N = 1 and N = 2
    assert {gc.graph(n).F - 1 for n in ("chain_n1", "chain_n2")} == {1, 2}


def test_graph_hooks_do_what_the_cases_need():
    # isolated: a free pose without any edge, and no coupling across it
    G = gc.graph("isolated")
    f = gc.CASES["isolated"]["args"]["extra"]["isolate"]
    assert not ((G.ii == f) | (G.jj == f)).any()
    st = gc.case_structure("isolated")
    assert all(not (b < f - 1 < a) for a, b in st["blocks"])  # relative id of frame f: f - 1
    assert (f - 1, f - 1) not in st["blocks"]
    # duplicates: some (kk, jj) pair occurs twice
    G = gc.graph("duplicates")
    pairs = np.stack([G.kk.numpy(), G.jj.numpy()], 1)
    assert len(np.unique(pairs, axis=0)) == G.E - 20
    # fixed prefix: edges among fixed frames, fixed -> free and free -> fixed
    G, t0 = gc.graph("fixed_prefix"), gc.CASES["fixed_prefix"]["t0"]
    ii, jj, kk = G.ii.numpy(), G.jj.numpy(), G.kk.numpy()
    assert ((ii < t0) & (jj < t0)).any() and ((ii < t0) & (jj >= t0)).any()
    assert ((ii >= t0) & (jj < t0)).any() and (ii == jj).any()
    fixed_only = [k for k in np.unique(kk) if ((ii[kk == k] < t0) & (jj[kk == k] < t0)).all()]
    assert fixed_only  # patches all of whose edges touch only fixed poses
    # edges are not grouped by patch
    assert (np.diff(gc.graph("g2").kk.numpy()) < 0).any()


@pytest.mark.parametrize("name", list(gc.CASES))
def test_oracle_agrees_with_structure_and_stays_off_the_clamps(name):
    c, st, G = gc.CASES[name], gc.case_structure(name), gc.graph(name)
    N = G.F - c["t0"]
    (_, K1, d1), (_, K2, d2) = _oracle(name, 1), _oracle(name, 2)
    assert d1["status"] == 0 and d2["status"] == 0
    # the oracle's dense S has nonzero 6 x 6 blocks exactly on the predicted
    # pattern (plus the damping's 1 on the diagonal of a pose without block)
    S = d1["S"].reshape(N, 6, N, 6)
    nz = np.abs(S).max(axis=(1, 3)) > 0
    want = np.zeros((N, N), bool)
    for a, b in st["blocks"]:
        want[a, b] = want[b, a] = True
    bare = [a for a in range(N) if not want[a, a]]
    for a in bare:
        assert np.array_equal(S[a, :, a, :], np.eye(6)) and not d1["y"][6 * a:6 * a + 6].any()
        want[a, a] = True
    assert np.array_equal(nz, want)
    # symmetric up to the summation order of its two triangles
    assert np.abs(d1["S"] - d1["S"].T).max() <= 1e-13 * np.abs(d1["S"]).max()
    zs = [K[:, 2] for K in (K1, K2)]
    print(f"\n{name}: (nI, nB, g, nsb)={c['expect']} largest set={st['maxset']} "
          f"cond(S)={np.linalg.cond(d1['S']):.3g} oracle status={d1['status']}/{d2['status']} "
          f"depth range it1=[{zs[0].min():.4g}, {zs[0].max():.4g}] "
          f"it2=[{zs[1].min():.4g}, {zs[1].max():.4g}] max|dX|={np.abs(d1['dX']).max():.3g}")
    if c["kind"] != "parity":
        return
    # clamp condition: no inverse depth sits on the 1e-4 floor or was reset to
    # 1 (d > 20) after either iteration, so GPU and oracle cannot fall on
    # different sides of a clamp
    for z in zs:
        assert not (z == np.float32(1e-4)).any() and not (z == 1.0).any() and z.max() < 19
    assert np.abs(d1["dX"]).max() > 1e-4  # the step is not trivially zero
