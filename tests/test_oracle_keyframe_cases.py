"""CPU: every case of tests/keyframe_cases.py reaches, on the oracle alone, the
branch of dpvo_amd/csrc/keyframe.hip it is named for (the conditions depend on
seeds: they are checked here, not assumed), and oracle.reduce_edges is pinned
against hand-made inputs.  test_keyframe_branches_gpu.py runs the same cases
on the device."""
import numpy as np
import pytest

import oracle
from keyframe_cases import (DROP_CASES, GRAPH_FRAMES, LOOP_CASES, build_drop, build_loop,
                            depth_after_transform, loop_window)

DROP_NAMES = [c["name"] for c in DROP_CASES]
LOOP_NAMES = [c["name"] for c in LOOP_CASES]


def test_case_names_are_unique():
    assert len(set(DROP_NAMES)) == len(DROP_NAMES)
    assert len(set(LOOP_NAMES)) == len(LOOP_NAMES)


# --------------------------------------------------------------------------- frame drop
@pytest.mark.parametrize("name", DROP_NAMES)
def test_drop_case_reaches_its_branch(name):
    b = build_drop(name)
    c, st, steps = b["case"], b["state"], b["steps"]
    n, KI, M, N = c["n"], c["KI"], c["M"], c["N"]
    i, j, k = n - KI - 1, n - KI + 1, n - KI
    assert N <= 48 and M <= 4 and n < N  # row n is read by nobody, but exists
    E = st["num_edges"]
    ii, jj = st["ii"][:E], st["jj"][:E]
    nfwd, nrev = int(((ii == i) & (jj == j)).sum()), int(((ii == j) & (jj == i)).sum())
    rs, info = steps[0]
    m0, m1 = info["mag"]
    if not c["graph"]:
        assert info["drop"] == c["expect_drop"], (m0, m1)
        assert info["k"] == k
    # every ring is the smallest supported size or larger
    for r in b["rings"].values():
        assert r == 0 or r > KI - 1

    if name.startswith("ki") and "moves" in name:
        nm = {"ki1_moves_0_frames": 0, "ki2_moves_1_frame": 1, "ki4_moves_3_frames": 3,
              "ki17_moves_16_frames": 16}[name]
        assert n - 1 - k == nm == KI - 1
        assert rs["n"] == n - 1 and rs["num_edges"] < E  # edges and counters change for KI = 1 too
        if nm == 0:
            for a in ("poses", "patches", "intrinsics", "tstamps"):
                np.testing.assert_array_equal(rs[a], st[a])
        else:
            assert not np.array_equal(rs["poses"], st["poses"])
        if nm == 16:
            assert b["rings"]["gmap"] == 17 and k % 17 + 16 >= 17  # the ring rows wrap
    elif name == "ki4_large_motion_is_kept":
        assert nfwd and nrev and (float(m0) + float(m1)) / 2 > 12.5
        assert rs["n"] == n and rs["num_edges"] == E
    elif name == "n_eq_ki_has_no_candidate":
        assert i == -1 and m0 == 0 and m1 == 0  # below the threshold, and still no drop
    elif name == "edges_i_to_j_only":
        assert nfwd > 0 and nrev == 0 and m0 > 0 and m1 == 0
    elif name == "edges_j_to_i_only":
        assert nfwd == 0 and nrev > 0 and m0 == 0 and m1 > 0
    elif name == "edges_neither_is_a_drop":
        assert nfwd == 0 and nrev == 0 and m0 == 0 and m1 == 0 and E > 0
    elif name.startswith("edge_count_"):
        assert E == c["E"] == int(name.rsplit("_", 1)[1])
        if E >= 1:
            assert nfwd > 0 and m0 > 0
        if E >= 2:
            assert (ii[E - 1], jj[E - 1]) == (j, i) and m1 > 0  # the last edge counts
            assert ((ii == k) | (jj == k)).sum() > 0 and rs["num_edges"] < E
    elif name.startswith("thresh_"):
        mid = (float(m0) + float(m1)) / 2
        assert mid > 0
        assert b["thresh"] == (mid if name == "thresh_equal_is_kept" else np.nextafter(mid, np.inf))
    elif name == "clamped_projection":
        sel = (ii == i) & (jj == j)
        Z = depth_after_transform(st["poses"], st["patches"], st["intrinsics"], ii[sel], jj[sel],
                                  st["kk"][:E][sel])
        assert (Z < 0.09).sum() > 0, "no pixel takes the fmaxf(Z, 0.1) clamp"
        assert ((Z > 0.11) & (Z < 0.19)).sum() > 0
        assert (Z > 0.25).sum() > 0
        assert (np.abs(Z - 0.2) > 1e-3).all() and (np.abs(Z - 0.1) > 1e-3).all()
        _, val = oracle.flow_mag(st["poses"], st["patches"], st["intrinsics"], ii[sel], jj[sel],
                                 st["kk"][:E][sel], 0.5)
        np.testing.assert_array_equal(val, Z > 0.2)  # the oracle sees the same depths
        qn = np.linalg.norm(st["poses"][:, 3:].astype(np.float64), axis=1)
        assert (np.abs(qn - 1.001) < 1e-5).all()
        assert np.isfinite(m0) and m0 > 12.5
    elif name.startswith("patch_"):
        assert c["P"] == {"patch_1x1": 1, "patch_2x2": 2, "patch_4x4": 4}[name]
        assert st["patches"].shape[-1] == c["P"] and m0 > 0 and m1 > 0
    elif name == "ring_min_rows_wrap":
        for r in b["rings"].values():
            assert r == KI == (n - 1 - k) + 1
            rows = [f % r for f in range(k, n)]
            assert rows != sorted(rows)  # the moved rows wrap around the end of the ring
    elif name == "ring_much_larger_than_n":
        assert min(b["rings"].values()) > 20 * n
    elif name.startswith("frame_bytes_"):
        a = st["a"]
        assert a[0].nbytes == int(name.split("_")[2])
        if "fp16" in name:
            assert a.dtype == np.float16
        assert not np.array_equal(rs["a"], a)
    elif name == "frame_int64":
        assert st["a"].dtype == np.int64 and not np.array_equal(rs["a"], st["a"])
    elif name == "twelve_arrays":
        assert 4 + len(c["frames"]) == 12
        assert {st[f[0]].dtype for f in c["frames"]} == {np.dtype(t) for t in
                                                         (np.float32, np.uint8, np.int64, np.float16)}
    elif name == "two_drops_in_a_row":
        assert len(steps) == 2 and steps[0][1]["drop"] and steps[1][1]["drop"]
        assert steps[1][0]["n"] == n - 2
    elif name == "two_drops_graph_replay":
        drops = [s[1]["drop"] for s in steps]
        assert len(drops) == 2 * GRAPH_FRAMES
        assert sum(drops) >= 2 and not all(drops), drops
        # at least one decision made from edges in both directions on either side
        assert any(s[1]["drop"] and s[1]["mag"][0] > 0 for s in steps)
        assert any(not s[1]["drop"] for s in steps)
        assert steps[-1][0]["n"] < N
    else:
        raise AssertionError(f"case {name} has no branch check")


# --------------------------------------------------------------------------- edges_loop
def _reduce_inputs(b):
    g, thr = b["groups"], np.float32(b["par"]["backend_thresh"])
    mask = g["fm"] < thr
    return g["fm"][mask], g["gi"][mask], g["gj"][mask]


@pytest.mark.parametrize("name", LOOP_NAMES)
def test_loop_case_reaches_its_branch(name):
    b = build_loop(name)
    c, par, g = b["case"], b["par"], b["groups"]
    n, M = c["n"], c["M"]
    ne = len(b["kk"]) // M
    assert M <= 4 or name.startswith(("patches_", "gate_M8"))
    assert par["global_opt_freq"] <= par["removal_window"] + 1 and par["keyframe_index"] >= 0
    assert {"edges": ne > 0, "none": ne == 0, "closed": ne == 0}[c["expect"]], ne
    assert (loop_window(c) is None) == (c["expect"] == "closed")
    if ne:
        assert ((b["jj"] - b["ix"][b["kk"]]) >= 30).all()
    if c["last"] is not None:
        assert b["last_after"] == (n if ne else c["last"])

    if name == "n_eq_removal_window":
        assert n - c["rw"] == 0 and g is None
    elif name == "n_eq_removal_window_plus_1":
        assert n - c["rw"] == 1 and g["nf"] == 1 and (g["gi"] == 0).all()
    elif name.startswith("max_edge_age_"):
        assert g["nf"] == c["age"] == int(name[-1]) and g["gi"].min() == n - c["rw"] - c["age"] > 0
    elif name == "gof_eq_keyframe_index_no_targets":
        assert c["gof"] == c["ki"] and g is None and n > c["rw"]
    elif name == "non_default_window":
        assert (c["rw"], c["gof"], c["ki"], c["age"]) == (9, 8, 2, 40)
        assert g["gi"].min() == 0 and g["nf"] == n - 9 and g["nj"] == 6
    elif name == "candidates_all_closer_than_30":
        fl, gi, gj = _reduce_inputs(b)
        assert len(fl) > 0 and (gj - gi < 30).all() and (fl < 1000).all()
    elif name == "thresh_eq_smallest_group_no_key":
        assert np.float32(par["backend_thresh"]) == g["fm"].min() and len(_reduce_inputs(b)[0]) == 0
        assert np.isfinite(g["fm"]).any()
    elif name == "thresh_next_above_smallest_one_key":
        assert len(_reduce_inputs(b)[0]) == 1 and ne == 1
    elif name.startswith("patches_"):
        assert M == int(name.split("_")[1])
        assert (g["cnt"] < M).any() or M == 1  # invalid patches occur: the count matters
    elif name.startswith("gate_M"):
        f, j, valid = c["gate"]
        sel = (g["gi"] == f) & (g["gj"] == j)
        assert sel.sum() == 1 and g["cnt"][sel][0] == valid
        lim = int(np.floor(0.75 * M))
        edge = bool(((b["ix"][b["kk"]] == f) & (b["jj"] == j)).any())
        if "is_inf" in name:
            assert valid == lim and np.isinf(g["fm"][sel][0]) and not edge
        else:
            assert valid == lim + 1 and g["fm"][sel][0] < par["backend_thresh"] and edge
    elif name.startswith("max_num_edges_"):
        free = len(oracle.edges_loop(b["poses"], b["patches"], b["intrinsics"], b["ix"], n, M,
                                     **dict(par, max_num_edges=1000))[0]) // M
        want = {"0": 0, "1": 1, "2": 2, "one": free - 1}[name.split("_")[3]]
        assert par["max_num_edges"] == want and ne == want and free > 3
    elif name.startswith("nms_"):
        by = {v: len(oracle.edges_loop(b["poses"], b["patches"], b["intrinsics"], b["ix"], n, M,
                                       **dict(par, nms=v))[0]) // M for v in (0, 1, 5, 1000)}
        assert by[0] > by[1] > by[5] > by[1000] >= 1, by  # each radius decides differently
        assert par["nms"] == {"0": 0, "1": 1, "5": 5, "larger": 1000}[name.split("_")[1]]
        assert par["nms"] < 1000 or par["nms"] > b["N"]
    elif name == "exact_tie_order":
        f = c["tie"]
        fl, gi, gj = _reduce_inputs(b)
        a, bb = np.flatnonzero(gi == f), np.flatnonzero(gi == f + 1)
        assert len(a) and len(a) == len(bb)
        np.testing.assert_array_equal(fl[a].view(np.uint32), fl[bb].view(np.uint32))  # the tie
        es = oracle.reduce_edges(fl, gi, gj, par["max_num_edges"], par["nms"])
        # the same candidates with every tie taken in the opposite order
        rev = oracle.reduce_edges(fl[::-1], gi[::-1], gj[::-1], par["max_num_edges"], par["nms"])
        assert {tuple(e) for e in es} != {tuple(e) for e in rev}
        E0, E1 = {tuple(e) for e in es}, {tuple(e) for e in rev}
        # some target frame where the tied pair is decided by its order alone
        assert any((f, j) in E0 and (f + 1, j) not in E0 and (f + 1, j) in E1 and (f, j) not in E1
                   for j in set(gj.tolist()))
    elif name.startswith("sort_ng_"):
        ng = int(name.split("_")[2])
        assert g["ng"] == ng
        p2 = 1 << max(ng - 1, 0).bit_length()
        assert p2 == {1: 1, 2: 2, 3: 4, 1023: 1024, 1024: 1024, 1025: 2048, 4400: 8192,
                      16384: 16384}[ng]
        if ng == 4400:
            assert ne == 596 and p2 // 2 > 1024  # several compare pairs per thread and step
    elif name == "gate_closed_one_frame_early":
        assert n - c["last"] == c["gof"] - 1
        assert len(oracle.edges_loop(b["poses"], b["patches"], b["intrinsics"], b["ix"], n, M,
                                     **par)[0]) > 0  # edges are there; only the gate is shut
    elif name == "gate_open_at_global_opt_freq":
        assert n - c["last"] == c["gof"]
    else:
        raise AssertionError(f"case {name} has no branch check")


# --------------------------------------------------------------------------- reduce_edges
def test_reduce_edges_dummy_entry_rule():
    """len(es) > max_num_edges with es holding a dummy: at most max_num_edges
    edges, none at 0."""
    fl = np.array([3.0, 1.0, 2.0], np.float32)
    ii, jj = np.array([0, 10, 20]), np.array([40, 50, 60])
    assert oracle.reduce_edges(fl, ii, jj, 0, 0).tolist() == []
    assert oracle.reduce_edges(fl, ii, jj, 1, 0).tolist() == [[10, 50]]
    assert oracle.reduce_edges(fl, ii, jj, 2, 0).tolist() == [[10, 50], [20, 60]]
    assert oracle.reduce_edges(fl, ii, jj, 3, 0).tolist() == [[10, 50], [20, 60], [0, 40]]


def test_reduce_edges_suppression_is_clipped_at_the_lookup():
    """ignore_lookup has ii.max() + 1 rows: i + nms beyond it (and i - nms
    below 0) is clipped, the neighbours inside are suppressed, other target
    frames are not."""
    fl = np.array([1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    ii, jj = np.array([9, 8, 0, 7, 8]), np.array([50, 50, 50, 50, 51])
    # (9, 50) first: suppresses (8, 50) and nothing above row 9; (0, 50) is far
    # away; (7, 50) is outside nms = 1; (8, 51) is another target frame
    assert oracle.reduce_edges(fl, ii, jj, 1000, 1).tolist() == [[9, 50], [0, 50], [7, 50], [8, 51]]
    assert oracle.reduce_edges(fl, ii, jj, 1000, 2).tolist() == [[9, 50], [0, 50], [8, 51]]
    assert oracle.reduce_edges(fl, ii, jj, 1000, 100).tolist() == [[9, 50], [8, 51]]


def test_reduce_edges_skips_close_pairs_and_large_flow():
    fl = np.array([1.0, 2.0, 3.0, 1000.0, 999.0], np.float32)
    ii, jj = np.array([21, 20, 0, 1, 2]), np.array([50, 50, 29, 60, 61])
    # j - i = 29 skipped twice (and a skipped pair suppresses nothing), = 30 taken;
    # flow >= 1000 skipped
    assert oracle.reduce_edges(fl, ii, jj, 1000, 1).tolist() == [[20, 50], [2, 61]]


def test_reduce_edges_stable_ties():
    fl = np.array([1.0, 1.0], np.float32)
    ii, jj = np.array([5, 4]), np.array([50, 50])
    assert oracle.reduce_edges(fl, ii, jj, 1000, 1).tolist() == [[5, 50]]
    assert oracle.reduce_edges(fl[::-1], ii[::-1], jj[::-1], 1000, 1).tolist() == [[4, 50]]
