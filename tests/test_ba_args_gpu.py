"""Argument validation of the cuda_ba BA / reprojection entries.

Every rejected call here is refused on the host, before any launch: a CPU
tensor in each tensor slot the entry checks, float64 poses, non-contiguous
poses (the in-place entries only; the reprojections copy), an int64 t0_dev
(the device-t0 entries only), and kk one element LONGER than ii.  The long kk
is harmless to the kernels (they read kk[e] for e < ii.numel() only), so the
case cannot read out of bounds even where an entry does not check it; it
passes only where ii / jj / kk are checked for one length, which the shared
edge-input helper now does for every entry.

Shapes: 4 poses, 6 patches of 3 x 3, 8 edges, window (1, 4).  The last test
runs one valid forward on the same inputs: the rejected calls left the status
machinery intact."""
import pytest
import torch

from dpvo_amd import synthetic

pytestmark = pytest.mark.gpu

T0, T1, N2 = 1, 4, 4
EDGE = ("poses", "patches", "intrinsics", "ii", "jj", "kk")
BA = ("poses", "patches", "intrinsics", "target", "weight", "lmbda", "ii", "jj", "kk")


@pytest.fixture(scope="module")
def cb(gpu):
    import dpvo_amd

    m = dpvo_amd.load_extension("cuda_ba")
    m.check_status(torch.zeros(1, device=gpu))  # clean slate
    return m


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
    return a


def _edge(a):
    return [a[k] for k in EDGE]


def _ba(a):
    return [a[k] for k in BA]


# name -> (call, tensor slots the entry checks, updates poses in place, reads t0_dev)
ENTRIES = {
    "forward": (lambda cb, a: cb.forward(*_ba(a), 1, T0, T1, 2, False), BA, True, False),
    "forward_dx": (lambda cb, a: cb.forward_dx(*_ba(a), 1, T0, T1, 2, False), BA, True, False),
    "forward_planned": (lambda cb, a: cb.forward_planned(a["ws"], *_ba(a), T0, T1, 2),
                        BA, True, False),
    "forward_planned_dev": (
        lambda cb, a: cb.forward_planned_dev(a["ws"], *_ba(a), a["t0_dev"], T1 - T0, 2),
        BA + ("t0_dev",), True, True),
    "reproject": (lambda cb, a: cb.reproject(*_edge(a)), EDGE, False, False),
    "reproject_ordered": (lambda cb, a: cb.reproject_ordered(*_edge(a), N2), EDGE, False, False),
    "reproject_ordered_plan": (lambda cb, a: cb.reproject_ordered_plan(*_edge(a), N2, T0, T1),
                               EDGE, False, False),
    "reproject_ordered_plan_insert": (
        lambda cb, a: cb.reproject_ordered_plan_insert(*_edge(a), N2, T0, T1, a["src"],
                                                       [a["dst0"], a["dst1"]], [1, 2]),
        EDGE + ("src", "dst0", "dst1"), False, False),
    "reproject_ordered_plan_dev": (
        lambda cb, a: cb.reproject_ordered_plan_dev(*_edge(a), N2, a["t0_dev"], T1 - T0),
        EDGE + ("t0_dev",), False, True),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_cpu_tensor_in_any_slot_is_rejected(cb, args, name):
    call, slots, _, _ = ENTRIES[name]
    for slot in slots:
        with pytest.raises(RuntimeError, match="GPU"):
            call(cb, dict(args, **{slot: args[slot].cpu()}))


@pytest.mark.parametrize("name", list(ENTRIES))
def test_float64_poses_are_rejected(cb, args, name):
    with pytest.raises(RuntimeError, match="float32"):
        ENTRIES[name][0](cb, dict(args, poses=args["poses"].double()))


@pytest.mark.parametrize("name", [n for n, e in ENTRIES.items() if e[2]])
def test_non_contiguous_poses_are_rejected_in_place(cb, args, name):
    wide = torch.zeros(4, 14, device=args["poses"].device)
    wide[:, :7] = args["poses"]
    nc = wide[:, :7]
    assert not nc.is_contiguous() and torch.equal(nc, args["poses"])
    with pytest.raises(RuntimeError, match=r"must be contiguous \(updated in place\)"):
        ENTRIES[name][0](cb, dict(args, poses=nc))


@pytest.mark.parametrize("name", [n for n, e in ENTRIES.items() if e[3]])
def test_int64_t0_dev_is_rejected(cb, args, name):
    with pytest.raises(RuntimeError, match="int32"):
        ENTRIES[name][0](cb, dict(args, t0_dev=args["t0_dev"].long()))


@pytest.mark.parametrize("name", list(ENTRIES))
def test_kk_longer_than_ii_is_rejected(cb, args, name):
    kk = torch.cat([args["kk"], args["kk"][-1:]])
    assert kk.numel() == args["ii"].numel() + 1
    with pytest.raises(RuntimeError, match="kk"):
        ENTRIES[name][0](cb, dict(args, kk=kk))


def test_valid_forward_after_the_rejections(cb, args):
    poses, patches = args["poses"].clone(), args["patches"].clone()
    cb.forward(*_ba(dict(args, poses=poses, patches=patches)), 1, T0, T1, 2, False)
    assert cb.check_status(poses) == 0
    assert not torch.equal(poses[T0:T1], args["poses"][T0:T1])  # the free poses moved
    assert torch.equal(poses[:T0], args["poses"][:T0])
