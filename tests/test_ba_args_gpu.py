"""Argument validation of the cuda_ba BA / reprojection entries, and of the
patch-graph, keyframe, tracker, BA-layer and transform entries next to them.

Every rejected call here is refused on the host, before any launch: a CPU
tensor in each tensor slot the entry checks, float64 poses (float16 poses for
the BA layer, which accepts float64), non-contiguous poses (the in-place
entries only; the reprojections copy), an int64 t0_dev (the device-t0 entries
only), kk one element LONGER than ii, and a [::2] view of a twice-as-long
buffer in each in-place buffer of the patch-graph and keyframe entries (a
one-element buffer has no such view: torch calls it contiguous).  The long kk
is harmless to the kernels (they read kk[e] for e < ii.numel() only), so the
case cannot read out of bounds even where an entry does not check it; it
passes only where ii / jj / kk are checked for one length, which the shared
edge-input helper now does for every entry.

Shapes: 4 poses, 6 patches of 3 x 3, 8 edges, window (1, 4); the patch-graph
store holds max_edges = 16 edges with DIM = 16 and counts of 3 words, which is
too short for the removals (they keep two scratch words there): those are only
ever refused here.  The last tests run one valid forward, pg_append and
kf_motion on the same inputs: the rejected calls left the status machinery and
the buffers intact, and the results are those of the same calls made before
the rejections."""
from typing import Callable, NamedTuple, Optional, Tuple

import pytest
import torch

from dpvo_amd import synthetic

pytestmark = pytest.mark.gpu

T0, T1, N2 = 1, 4, 4
EDGE = ("poses", "patches", "intrinsics", "ii", "jj", "kk")
BA = ("poses", "patches", "intrinsics", "target", "weight", "lmbda", "ii", "jj", "kk")
STORE = ("ii", "jj", "kk", "net", "weight", "target")
ACT = tuple("act_" + k for k in STORE)
BACK = tuple("back_" + k for k in STORE)
INAC = tuple("inac_" + k for k in STORE if k != "net")
LIVE = ACT[:4]  # the live edge arrays of the append entries: ii, jj, kk, net


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    m = dpvo_amd.load_extension("cuda_ba")
    m.check_status(torch.zeros(1, device=gpu))  # clean slate
    return m


def _append(cb, a):
    cb.pg_append(a["ix"], a["kk"], a["jj"], *[a[k] for k in LIVE], a["counts"])


def _kf_motion(cb, a):
    cb.kf_motion(*[a[k] for k in ACT[:3]], a["counts"], a["poses"], a["patches"], a["intrinsics"],
                 a["st"], 2, 12.5, a["kf"], a["mag"])


def _valid_graph_calls(cb, args):
    """One valid pg_append into a copy of the empty store, then kf_motion on it
    (frames 1 and 3 of 4): everything they wrote, as bits."""
    a = dict(args, **{k: args[k].clone() for k in LIVE + ("counts", "kf", "mag")})
    _append(cb, a)
    _kf_motion(cb, a)
    torch.cuda.synchronize()
    return [a[k].clone().view(torch.uint8) for k in LIVE + ("counts", "kf", "mag")]


@pytest.fixture(scope="module")
def args(cb, gpu):
    G = synthetic.make_graph(F=4, M=1, E=8, seed=5, num_patches=6)
    assert G.poses.shape == (4, 7) and G.patches.shape == (6, 3, 3, 3) and G.E == 8
    D = G.to(gpu)
    a = {k: getattr(D, k) for k in BA if k != "lmbda"}
    a["lmbda"] = torch.tensor([1e-4], device=gpu)
    a["t0_dev"] = torch.tensor([T0], dtype=torch.int32, device=gpu)
    a["ws"] = cb.plan(a["ii"], a["jj"], a["kk"], 6, 4, T0, T1)
    a["src"] = torch.zeros(8, 8, 8, device=gpu)  # [C, H, W]
    a["dst0"] = torch.zeros(8, 8, 8, device=gpu).permute(2, 0, 1)  # channels-last [C, H, W]
    a["dst1"] = torch.zeros(4, 4, 8, device=gpu).permute(2, 0, 1)

    def i64(*s):
        return torch.zeros(*s, dtype=torch.long, device=gpu)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=gpu)

    def f32(*s):
        return torch.zeros(*s, device=gpu)

    # the patch-graph edge stores: max_edges 16, DIM 16
    for p in ("act_", "back_", "inac_"):
        a.update({p + "ii": i64(16), p + "jj": i64(16), p + "kk": i64(16),
                  p + "weight": f32(1, 16, 2), p + "target": f32(1, 16, 2)})
        if p != "inac_":
            a[p + "net"] = f32(1, 16, 16)
    a["counts"], a["pos"] = i32([0, 0, 0]), i32([0] * 16)
    a["ix"] = torch.tensor([0, 0, 1, 2, 3, 3], device=gpu)  # the frame of each patch
    a["mask"] = torch.zeros(16, dtype=torch.bool, device=gpu)
    a["n_dev"] = i32([8])
    a["st"], a["kf"], a["mag"] = i32([4, 6]), i32([0, 0]), f32(2)
    a["tstamps"] = torch.arange(4, device=gpu)
    a["delta_log"], a["delta_tstamps"], a["delta_count"] = f32(8, 7), i64(8, 2), i32([0])
    a["work"] = f32(cb.edges_loop_work_floats())
    a["out_kk"], a["out_jj"], a["out_n"] = i64(4), i64(4), i32([0])
    a["last_global_ba"], a["errors"] = i32([0]), i32([0])
    a["points"], a["m_dev"] = f32(6, 3), i32([6])
    a["coords"], a["delta"], a["w"], a["E_dev"] = f32(1, 8, 2, 3, 3), f32(8, 2), f32(8, 2), i32([8])
    a["g_coords"] = f32(8, 3, 3, 2)
    a["before"] = _valid_graph_calls(cb, a)
    return a


def _edge(a):
    return [a[k] for k in EDGE]


def _ba(a):
    return [a[k] for k in BA]


def _stores(a, *which):
    return [[a[k] for k in s] for s in which]


class Row(NamedTuple):
    call: Callable
    slots: Tuple[str, ...]            # the tensor slots the entry checks
    in_place: bool = False            # updates poses in place
    t0_dev: bool = False              # reads t0_dev
    poses: Optional[str] = "float32"  # accepted poses dtype ("layer": float32 / float64), None: no such slot
    kk: bool = True                   # takes kk next to ii / jj
    buffers: Tuple[str, ...] = ()     # in-place buffers of more than one element


ENTRIES = {
    "forward": Row(lambda cb, a: cb.forward(*_ba(a), 1, T0, T1, 2, False), BA, True),
    "forward_dx": Row(lambda cb, a: cb.forward_dx(*_ba(a), 1, T0, T1, 2, False), BA, True),
    "forward_planned": Row(lambda cb, a: cb.forward_planned(a["ws"], *_ba(a), T0, T1, 2), BA, True),
    "forward_planned_dev": Row(
        lambda cb, a: cb.forward_planned_dev(a["ws"], *_ba(a), a["t0_dev"], T1 - T0, 2),
        BA + ("t0_dev",), True, True),
    "reproject": Row(lambda cb, a: cb.reproject(*_edge(a)), EDGE),
    "reproject_ordered": Row(lambda cb, a: cb.reproject_ordered(*_edge(a), N2), EDGE),
    "reproject_ordered_plan": Row(lambda cb, a: cb.reproject_ordered_plan(*_edge(a), N2, T0, T1),
                                  EDGE),
    "reproject_ordered_plan_insert": Row(
        lambda cb, a: cb.reproject_ordered_plan_insert(*_edge(a), N2, T0, T1, a["src"],
                                                       [a["dst0"], a["dst1"]], [1, 2]),
        EDGE + ("src", "dst0", "dst1")),
    "reproject_ordered_plan_dev": Row(
        lambda cb, a: cb.reproject_ordered_plan_dev(*_edge(a), N2, a["t0_dev"], T1 - T0),
        EDGE + ("t0_dev",), False, True),
    # ---- patch graph and keyframe: the new edges are the graph's kk / jj ----
    "pg_append": Row(_append, ("ix", "kk", "jj") + LIVE + ("counts",), poses=None,
                     buffers=LIVE + ("counts",)),
    "pg_append_dev": Row(
        lambda cb, a: cb.pg_append_dev(a["ix"], a["kk"], a["jj"], a["n_dev"],
                                       *[a[k] for k in LIVE], a["counts"]),
        ("ix", "kk", "jj", "n_dev") + LIVE + ("counts",), poses=None, buffers=LIVE + ("counts",)),
    "pg_remove": Row(
        lambda cb, a: cb.pg_remove(a["mask"], a["ix"], 0, -1, False, *_stores(a, ACT, BACK, INAC),
                                   a["counts"], a["pos"]),
        ("mask", "ix") + ACT + BACK + INAC + ("counts", "pos"), poses=None, kk=False,
        buffers=ACT + BACK + INAC + ("counts", "pos")),
    "pg_remove_window_dev": Row(
        lambda cb, a: cb.pg_remove_window_dev(a["ix"], a["n_dev"], -2, -1, False, False,
                                              *_stores(a, ACT, BACK, INAC), a["counts"], a["pos"]),
        ("ix", "n_dev") + ACT + BACK + INAC + ("counts", "pos"), poses=None, kk=False,
        buffers=ACT + BACK + INAC + ("counts", "pos")),
    "pg_remove_frame_dev": Row(
        lambda cb, a: cb.pg_remove_frame_dev(a["kf"], *_stores(a, ACT, BACK), a["counts"],
                                             a["pos"]),
        ("kf",) + ACT + BACK + ("counts", "pos"), poses=None, kk=False,
        buffers=("kf",) + ACT + BACK + ("counts", "pos")),
    "kf_motion": Row(_kf_motion, ACT[:3] + ("counts", "poses", "patches", "intrinsics", "st", "kf",
                                            "mag"),
                     kk=False, buffers=("counts", "poses", "patches", "intrinsics", "st", "kf", "mag")),
    "kf_shift": Row(
        lambda cb, a: cb.kf_shift(a["kf"], 1, a["st"], *[a[k] for k in ACT[:3]], a["counts"],
                                  [a["poses"], a["intrinsics"]], [0, 0]),
        ("kf", "st") + ACT[:3] + ("counts", "poses", "intrinsics"), poses=None, kk=False,
        buffers=("kf", "st") + ACT[:3] + ("counts", "poses", "intrinsics")),
    "kf_shift_delta_log": Row(
        lambda cb, a: cb.kf_shift(a["kf"], 1, a["st"], *[a[k] for k in ACT[:3]], a["counts"],
                                  [a["intrinsics"]], [0], a["poses"], a["tstamps"], a["delta_log"],
                                  a["delta_tstamps"], a["delta_count"]),
        ("kf", "st") + ACT[:3] + ("counts", "intrinsics", "poses", "tstamps", "delta_log",
                                  "delta_tstamps", "delta_count"),
        kk=False, buffers=("kf", "st") + ACT[:3] + ("counts", "intrinsics", "poses", "tstamps",
                                                    "delta_log", "delta_tstamps")),
    "edges_loop": Row(
        lambda cb, a: cb.edges_loop(a["poses"], a["patches"], a["intrinsics"], a["ix"], 1, a["st"],
                                    4, a["last_global_ba"], 2, 1000, 2, 1, 64.0, 4, 1, a["work"],
                                    a["out_kk"], a["out_jj"], a["out_n"], a["errors"]),
        ("poses", "patches", "intrinsics", "ix", "st", "last_global_ba", "work", "out_kk", "out_jj",
         "out_n", "errors"),
        kk=False, buffers=("poses", "patches", "intrinsics", "work", "out_kk", "out_jj")),
    # ---- tracker, BA layer, transforms ----
    "map_points": Row(
        lambda cb, a: cb.map_points(a["poses"], a["patches"], a["intrinsics"], a["ix"], a["points"],
                                    6, a["m_dev"]),
        ("poses", "patches", "intrinsics", "ix", "points", "m_dev"), kk=False),
    "update_targets": Row(
        lambda cb, a: cb.update_targets(a["coords"], a["delta"], a["w"], a["target"], a["weight"],
                                        8, a["E_dev"]),
        ("coords", "delta", "w", "target", "weight", "E_dev"), poses=None, kk=False),
    "ba_layer_forward": Row(
        lambda cb, a: cb.ba_layer_forward(*[a[k] for k in BA[:6]], 1e-4, a["ii"], a["jj"], a["kk"],
                                          4, 1, False, [0.0, 0.0, 64.0, 48.0], 0.1, False),
        BA, poses="layer"),
    "transform_forward": Row(lambda cb, a: cb.transform_forward(*_edge(a), False), EDGE),
    "transform_backward": Row(
        lambda cb, a: cb.transform_backward(*_edge(a), a["g_coords"], True, True),
        EDGE + ("g_coords",)),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_cpu_tensor_in_any_slot_is_rejected(cb, args, name):
    row = ENTRIES[name]
    for slot in row.slots:
        with pytest.raises(RuntimeError, match="GPU"):
            row.call(cb, dict(args, **{slot: args[slot].cpu()}))


@pytest.mark.parametrize("name", [n for n, e in ENTRIES.items() if e.poses == "float32"])
def test_float64_poses_are_rejected(cb, args, name):
    with pytest.raises(RuntimeError, match="float32"):
        ENTRIES[name].call(cb, dict(args, poses=args["poses"].double()))


@pytest.mark.parametrize("name", [n for n, e in ENTRIES.items() if e.poses == "layer"])
def test_float16_poses_are_rejected_by_the_ba_layer(cb, args, name):
    with pytest.raises(RuntimeError, match="float32 or float64"):
        ENTRIES[name].call(cb, dict(args, poses=args["poses"].half()))


@pytest.mark.parametrize("name", [n for n, e in ENTRIES.items() if e.in_place])
def test_non_contiguous_poses_are_rejected_in_place(cb, args, name):
    wide = torch.zeros(4, 14, device=args["poses"].device)
    wide[:, :7] = args["poses"]
    nc = wide[:, :7]
    assert not nc.is_contiguous() and torch.equal(nc, args["poses"])
    with pytest.raises(RuntimeError, match=r"must be contiguous \(updated in place\)"):
        ENTRIES[name].call(cb, dict(args, poses=nc))


@pytest.mark.parametrize("name", [n for n, e in ENTRIES.items() if e.buffers])
def test_strided_view_of_an_in_place_buffer_is_rejected(cb, args, name):
    row = ENTRIES[name]
    for slot in row.buffers:
        t = args[slot]
        nc = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)[::2]
        assert nc.numel() == t.numel() > 1 and not nc.is_contiguous()
        with pytest.raises(RuntimeError, match="must be contiguous"):
            row.call(cb, dict(args, **{slot: nc}))


@pytest.mark.parametrize("name", [n for n, e in ENTRIES.items() if e.t0_dev])
def test_int64_t0_dev_is_rejected(cb, args, name):
    with pytest.raises(RuntimeError, match="int32"):
        ENTRIES[name].call(cb, dict(args, t0_dev=args["t0_dev"].long()))


@pytest.mark.parametrize("name", [n for n, e in ENTRIES.items() if e.kk])
def test_kk_longer_than_ii_is_rejected(cb, args, name):
    kk = torch.cat([args["kk"], args["kk"][-1:]])
    assert kk.numel() == args["ii"].numel() + 1
    with pytest.raises(RuntimeError, match="kk"):
        ENTRIES[name].call(cb, dict(args, kk=kk))


def test_valid_graph_calls_after_the_rejections(cb, args):
    """No refused call wrote to the shared store; pg_append and kf_motion give
    the bits they gave before the refusals."""
    for k in LIVE + ("counts", "kf"):
        assert not args[k].any(), k
    for got, want in zip(_valid_graph_calls(cb, args), args["before"]):
        assert torch.equal(got, want)
    counts = args["before"][len(LIVE)].view(torch.int32)
    assert counts.tolist() == [8, 0, 0]  # the eight edges went in


def test_valid_forward_after_the_rejections(cb, args):
    poses, patches = args["poses"].clone(), args["patches"].clone()
    cb.forward(*_ba(dict(args, poses=poses, patches=patches)), 1, T0, T1, 2, False)
    assert cb.check_status(poses) == 0
    assert not torch.equal(poses[T0:T1], args["poses"][T0:T1])  # the free poses moved
    assert torch.equal(poses[:T0], args["poses"][:T0])
