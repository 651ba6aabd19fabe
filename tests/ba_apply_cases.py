"""Case table of test_ba_window_apply_gpu.py and scripts/make_ba_apply_golden.py:
the shapes at which the BA window kernel's apply step (ba_window.hip apply_dx:
a solved dX -> new poses and inverse depths, between iterations and after the
last one) can go wrong.  The graphs come from the builders of ba_setup_cases.py
and ba_gates.py; nothing is generated here.

The apply step gives the poses to threads 0 .. N-1 and relevant patch ri of a
workgroup to thread (64 + ri) mod 256, so the counts that matter are those of
ONE workgroup.  Two kinds of case pin them down on the host:
  structure only (t0 == t1): one workgroup, every patch relevant and owned;
  N = 1: four workgroups (the diagonal block's shares); workgroup s takes the
         patches that see the free pose with (index mod 4) == s, workgroup 0
         also every patch without a free pose (relevant_counts_n1).
"""
import numpy as np

import ba_gates
from ba_setup_cases import BA_CASES, _graph, patch_masks


def relevant_counts_n1(G, t0):
    """Relevant patches of each of the 4 workgroups of a window with one free
    pose (ba_window.hip: rel(u), u the patch's rank in ascending patch id)."""
    m = patch_masks(G.ii.numpy(), G.jj.numpy(), G.kk.numpy(), t0, t0 + 1)
    u = np.arange(m.size)
    return [int(((m != 0) & (u % 4 == s)).sum() + (int((m == 0).sum()) if s == 0 else 0))
            for s in range(4)]


def _setup(name, iters):
    G, t0, t1, _ = BA_CASES[name]()
    return G, t0, t1, iters


def _gate(name):
    G, _, t0, t1 = ba_gates.case(name)
    return G, t0, t1, ba_gates.ITERS


# name -> (Graph, t0, t1, iterations)
CASES = {
    # iterations: 1 = only the final apply; 2 = one in-loop apply; 3 = the in-loop
    # apply takes its base from dbase first, then from dep.  N = 11: the benchmark's size
    "N11_it1": lambda: _setup("N11", 1),
    "N11_it2": lambda: _setup("N11", 2),
    "N11_it3": lambda: _setup("N11", 3),
    # free poses.  From N = 2 on the off-diagonal workgroups own none of their
    # relevant patches (pkx < 0): only owned ones may be stored
    "N1_it2": lambda: _setup("N1", 2),
    "N2_it2": lambda: _setup("N2", 2),
    "N2_it3": lambda: _setup("N2", 3),
    "N16_it2": lambda: _setup("N16", 2),
    # no free pose: the NB == 0 structure-only path, dZ = Q u
    "N0_it1": lambda: _setup("N0", 1),
    "N0_it3": lambda: _setup("N0", 3),
    # t0 > 1: edges touch fixed poses; patches without a free pose go to workgroup 0
    "t0_9": lambda: _setup("no_free_pose_patches", 2),
    "t0_70_hbm_fixed_poses": lambda: _setup("hbm_fixed_poses", 2),
    "E2048_cfg2_shape": lambda: _setup("E2048", 2),
    # relevant patches of one workgroup: 144 (< 192: no wrap), exactly 192 and 193
    # (patch 192 wraps onto thread 0), 320 (the stride loop runs twice); one edge per patch
    "struct_192": lambda: (_graph(F=25, M=8, E=192, seed=41), 1, 1, 2),
    "struct_193": lambda: (_graph(F=25, M=8, E=193, seed=41), 1, 1, 2),
    "struct_320": lambda: (_graph(F=40, M=8, E=400, seed=42), 1, 1, 3),
    # the same counts in workgroup 0 of a window with one free pose: thread 0
    # retracts the pose AND takes the wrapped patch (counts asserted by the test)
    "N1_wg0_192": lambda: (_graph(F=30, M=8, E=N1_E[192], seed=43), 1, 2, 2),
    "N1_wg0_193": lambda: (_graph(F=30, M=8, E=N1_E[193], seed=43), 1, 2, 3),
    # 2304 patches: workgroup 0 has more relevant patches than the region holds
    # kTP parts for -> the one-thread-per-patch fallback with the E entries in HBM
    "nuniq_gt_2048": lambda: _setup("nuniq_gt_2048", 2),
    # DPVO's window (E = 9600, ~10 edges per patch): E entries in the shared HBM
    # buffer, the kTP path of the final apply
    "dpvo_n10_it1": lambda: _setup("dpvo_n10_it1", 1),
    "dpvo_n10_it2": lambda: _setup("dpvo_n10_it2", 2),
    "dpvo_n10_it3": lambda: _setup("dpvo_n10_it2", 3),
    # clamps: depths pushed above 20 (reset to 1; the late patches in the second
    # iteration, i.e. by the final apply) and below 1e-4 (the floor)
    "gates_cfg1": lambda: _gate("cfg1"),
    "gates_struct": lambda: _gate("struct"),
    "gates_dpvo10": lambda: _gate("dpvo10"),
    # patch size: the direct stores write P * P copies per patch.  P = 2 is the
    # smallest patch the window path accepts (it reads element [1][1]); P = 1
    # is refused by plan_supported and never reaches this kernel
    "P2": lambda: (_graph(F=18, M=8, E=300, seed=44, p=2), 1, 12, 2),
    "P3": lambda: (_graph(F=18, M=8, E=300, seed=44, p=3), 1, 12, 2),
}

# edge counts at which workgroup 0 of the N = 1 window over _graph(F=30, M=8,
# seed=43) has exactly that many relevant patches (relevant_counts_n1; found by
# trying E = 180 .. 400 on the host)
N1_E = {192: 201, 193: 202}

# what the test asserts about the host-countable cases: relevant patches per workgroup
STRUCT_COUNTS = {"struct_192": 192, "struct_193": 193, "struct_320": 320, "N0_it1": 144,
                 "N0_it3": 144}
N1_COUNTS = {"N1_wg0_192": 192, "N1_wg0_193": 193}


def run(G, t0, t1, iters, dev):
    """fastba.BA on a planned workspace (the window path) -> poses, patches,
    the last iteration's dX [N, 6] (fp64), the call's status."""
    import torch

    from dpvo_amd import fastba

    cb = fastba.cuda_ba
    D = G.to(dev)
    P = int(D.patches.shape[-1])
    assert cb.plan_supported(G.E, t0, t1, P), "not a window-path shape"
    ws = fastba.plan(D.ii, D.jj, D.kk, t0, t1, D.patches.shape[0], D.poses.shape[0], P=P)
    assert ws is not None
    poses, patches = D.poses.clone(), D.patches.clone()
    fastba.BA(poses, patches, D.intrinsics, D.target, D.weight, torch.tensor([1e-4], device=dev),
              D.ii, D.jj, D.kk, t0, t1, M=G.M, iterations=iters, plan=ws)
    dX = cb.last_dx(ws, G.E, t0, t1).cpu().numpy()
    status = cb.check_status(poses)
    return poses.cpu().numpy(), patches.cpu().numpy(), dX, status

# cases whose result holds depths reset to 1 (from above 20) and depths at the floor 1e-4
CLAMPED = ("gates_cfg1", "gates_struct", "gates_dpvo10")
