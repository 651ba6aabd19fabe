"""Graph builder, band-structure restatement and case table of the large-graph
F-BA branch tests (test_oracle_gba_cases.py on the CPU,
test_ba_large_branches_gpu.py on the GPU).

ba_large.hip chooses its code by the graph's structure: the superblock size
g (m = 6 g rows: panel tails, the one- or two-product staging of k_cr_b /
k_cr_back), the superblock count nsb (which neighbours exist at each level of
the cyclic reduction), the border size nB (register or in-HBM Gauss-Jordan,
the partial-sum loop of the border Schur complement) and the limits that set
a status bit.  A test that means to run one branch has to prove that its graph
reaches it: `chain_graph` builds graphs whose structure can be read off their
arguments, `structure` restates the band analysis (from the comment at the top
of ba_large.hip, not from its kernels), and `CASES` writes the structure every
case is for as literals, which the CPU test checks against `structure` and
against the oracle's dense S.  No GPU, no test functions.

A new solver branch gets a row in `CASES` (and, if it depends on a new
structural quantity, a column in `branches`)."""
import numpy as np
import torch

from dpvo_amd import synthetic

GCAP = 16        # ba_bgj.hpp kGCap: a coupling further back than this -> border
MAX_SET = 24     # ba_large.hip kMaxSet
MAX_BORDER = 64  # ba_large.hip kMaxBorder
MAX_M = 6 * GCAP
BP = 32          # ba_large.hip kBP: border Schur partial groups
# status bits of ba_large.hip
ST_CHOL, ST_CLAMP, ST_SET, ST_BORDER = 1, 2, 4, 8


def chain_graph(F, M, offsets, far=(), seed=0, noise=0.02, extra=None):
    """Poses, patches and intrinsics of synthetic.make_graph_large(F, M, 0, 0,
    seed) (periodic trajectory: far edges stay in front of the camera) with a
    prescribed edge set: every patch k of frame i = k // M gets an edge to
    frame i + d for each d in `offsets` inside [0, F); each (src, dst, n) of
    `far` adds edges from the first n patches of frame src to frame dst.
    extra: dict of hooks, applied in this order
      "fixed":   [(src, dst, n), ...] more edges of the `far` form (meant for
                 pairs of frames below t0)
      "isolate": frame f: every edge from a patch of f or to f is dropped
      "dup":     (lo, hi): edges [lo, hi) of the list so far are appended again
                 (same patch and frames; their own target noise and weight)
    Targets: synthetic.reproject_centres + noise * N(0, 1) px; weights U(0, 1);
    edges in a seeded shuffled order."""
    extra = dict(extra or {})
    base = synthetic.make_graph_large(F, M, 0, 0, seed)
    kk, jj = [], []
    k_all = np.arange(F * M)
    for d in offsets:
        j = k_all // M + d
        ok = (j >= 0) & (j < F)
        kk.append(k_all[ok])
        jj.append(j[ok])
    for src, dst, n in list(far) + list(extra.pop("fixed", ())):
        assert 0 <= src < F and 0 <= dst < F and 0 < n <= M
        kk.append(src * M + np.arange(n))
        jj.append(np.full(n, dst))
    kk, jj = np.concatenate(kk), np.concatenate(jj)
    f = extra.pop("isolate", None)
    if f is not None:
        keep = (kk // M != f) & (jj != f)
        kk, jj = kk[keep], jj[keep]
    dup = extra.pop("dup", None)
    if dup is not None:
        kk = np.concatenate([kk, kk[dup[0]:dup[1]]])
        jj = np.concatenate([jj, jj[dup[0]:dup[1]]])
    assert not extra, f"unknown hooks {sorted(extra)}"
    r = np.random.default_rng(1000 + seed)
    perm = r.permutation(len(kk))
    kk, jj = kk[perm].astype(np.int64), jj[perm].astype(np.int64)
    ii = kk // M
    intr = base.intrinsics[0].tolist()
    ctr = synthetic.reproject_centres(base.poses.double().numpy(), base.patches.double().numpy(),
                                      intr, ii, jj, kk)
    target = (ctr + noise * r.standard_normal(ctr.shape)).astype(np.float32)
    weight = r.uniform(0, 1, ctr.shape).astype(np.float32)
    return synthetic.Graph(base.poses, base.patches, base.intrinsics, torch.from_numpy(ii),
                           torch.from_numpy(jj), torch.from_numpy(kk), torch.from_numpy(target),
                           torch.from_numpy(weight), F, M)


def lblk(a, b):
    """Index of lower block (a, b), a >= b (ba_device.hpp lblk): the packed S
    blocks are in ascending order of it."""
    assert a >= b
    return a * (a + 1) // 2 + b


def structure(ii, jj, kk, t0, t1):
    """Band analysis of the graph, restated: a patch's pose set is the free
    poses (relative ids in [0, t1 - t0)) among the ii and jj of its edges;
    every pair inside a set is a coupling (lower block (a, b), a >= b); a pose
    with a coupling more than GCAP poses back is border; the remaining poses
    are renumbered (compressed) in order; g is the largest compressed distance
    of a coupling between two interior poses, at least 1 and at most GCAP;
    nsb = ceil(nI / g).  Sets larger than MAX_SET and more than MAX_BORDER
    border poses are reported as they are: what the solver does then is its
    status path, not part of this restatement."""
    ii, jj, kk = (np.asarray(a).astype(np.int64).tolist() for a in (ii, jj, kk))
    N = max(t1 - t0, 0)
    sets = {}
    for i, j, k in zip(ii, jj, kk):
        s = sets.setdefault(k, set())
        for a in (i - t0, j - t0):
            if 0 <= a < N:
                s.add(a)
    blocks = set()
    for s in sets.values():
        for a in s:
            for b in s:
                if a >= b:
                    blocks.add((a, b))
    blocks = sorted(blocks, key=lambda ab: lblk(*ab))
    border = sorted({a for a, b in blocks if a - b > GCAP})
    bset = set(border)
    cidx, c = {}, 0
    for a in range(N):
        if a not in bset:
            cidx[a] = c
            c += 1
    nI, nB = N - len(border), len(border)
    g = 1
    for a, b in blocks:
        if a in cidx and b in cidx:
            g = max(g, cidx[a] - cidx[b])
    g = min(g, GCAP)
    return {"nuniq": len(sets), "nitems": sum(len(s) * (len(s) + 1) // 2 for s in sets.values()),
            "blocks": blocks, "nblk": len(blocks), "nI": nI, "nB": nB, "g": g,
            "nsb": -(-nI // g), "maxset": max((len(s) for s in sets.values()), default=0),
            "border": border, "cidx": cidx}


def level_counts(nsb):
    """Active superblocks at each level of the cyclic reduction (level 0 first,
    down to the single top superblock)."""
    out = [nsb]
    while out[-1] > 1:
        out.append((out[-1] + 1) // 2)
    return out


def two_fit(g):
    """k_cr_b / k_cr_back stage both products at once when their operands fit
    160 KiB of LDS (ba_large.hip two_fit): true up to g = 13."""
    m = 6 * g
    return 8 * (MAX_M * MAX_M + m * m + 2 * m * 32) <= 160 * 1024


def branches(st):
    """The solver branches a graph of this structure runs, as a set of names
    (derived from the structure alone)."""
    out = set()
    g, nsb, nB, nI = st["g"], st["nsb"], st["nB"], st["nI"]
    if nB > MAX_BORDER:
        return {"status_border"}
    if st["maxset"] > MAX_SET:
        out.add("status_set")
    out.add(f"g{g}")
    out.add("nsb>32" if nsb > BP else f"nsb{nsb}")
    out.add(f"nB{nB}" if nB in (0, 1, 16, 17, 64) else "nB_other")
    out.add("border_gj_hbm" if 6 * nB > MAX_M else ("border_gj_regs" if nB else "no_border"))
    if nB and nsb > BP:
        out.add("border_part_loop")
    if nI % g:
        out.add("padded_last_superblock")
    if st["maxset"] == MAX_SET:
        out.add("set24")
    # neighbours of the kept / eliminated superblocks at each reduction level,
    # and how the two-product workgroups stage their operands: k_cr_b forms two
    # products only for a kept superblock with both neighbours, k_cr_back only
    # for an eliminated one with a right neighbour; both at once if two_fit,
    # else one after the other through the same LDS.  With a single product the
    # code is the same for every g.
    staging = "two_fit" if two_fit(g) else "sequential"
    for n in level_counts(nsb):
        if n < 2:
            continue
        for k in range(0, n, 2):  # kept
            out.add("kept:" + ("l" if k >= 1 else "-") + ("r" if k + 1 < n else "-")
                    + ("R" if k + 2 < n else "-"))
            if k >= 1 and k + 1 < n:
                out.add("cr_b_both:" + staging)
        for k in range(1, n, 2):  # eliminated
            out.add("elim:" + ("r" if k + 1 < n else "-"))
            if k + 1 < n:
                out.add("cr_back_r:" + staging)
    # k_assemble's destinations.  In the kernel `ai` is "ab.x (the higher pose
    # a) is interior": true for an interior pose above a border pose, false for
    # a border pose above an interior one (the issue's text has the two swapped)
    cidx, border = st["cidx"], set(st["border"])
    for a, b in st["blocks"]:
        if a in cidx and b in cidx:
            out.add("asm_D" if cidx[a] // g == cidx[b] // g else "asm_L")
        elif a in cidx:
            out.add("asm_interior_above_border")  # k_assemble: ai true
        elif b in cidx:
            out.add("asm_border_above_interior")  # k_assemble: ai false
        else:
            out.add("asm_Cb_diag" if a == b else "asm_Cb_off")
    touched = {a for a, _ in st["blocks"]}
    if len(touched) < nI + nB:
        out.add("pose_without_block")
    return out


def _c(expect, kind="parity", t0=1, **args):
    return {"args": args, "t0": t0, "expect": expect, "kind": kind}


def _border(targets):
    return [(a - 20, a, 2) for a in targets]


# name -> builder arguments, t0 and the expected (nI, nB, g, nsb) as literals.
# kind "parity": status 0, full comparison with the oracle; kind "status": the
# graph exceeds a limit of the solver (the structure is the graph's own; what
# the solver reports then is asserted in the GPU test).
CASES = {
    # g = 1 chains (one edge per patch to the next frame): nsb = F - 1
    "chain_n1": _c((1, 0, 1, 1), F=2, M=4, offsets=(1,)),
    "chain_n2": _c((2, 0, 1, 2), F=3, M=4, offsets=(1,)),
    "chain_n3": _c((3, 0, 1, 3), F=4, M=4, offsets=(1,)),
    "chain_n4": _c((4, 0, 1, 4), F=5, M=4, offsets=(1,)),
    "chain_n5": _c((5, 0, 1, 5), F=6, M=4, offsets=(1,)),
    "chain_n6": _c((6, 0, 1, 6), F=7, M=4, offsets=(1,)),
    "chain_n7": _c((7, 0, 1, 7), F=8, M=4, offsets=(1,)),
    "chain_n9": _c((9, 0, 1, 9), F=10, M=4, offsets=(1,)),
    # superblock sizes: offsets (1, g) give couplings 1, g - 1 and g
    "g2": _c((6, 0, 2, 3), F=7, M=4, offsets=(1, 2)),
    "g5_pad": _c((14, 0, 5, 3), F=15, M=4, offsets=(1, 5)),
    "g13_pad": _c((37, 0, 13, 3), F=38, M=4, offsets=(1, 13)),
    "g14_pad": _c((40, 0, 14, 3), F=41, M=4, offsets=(1, 14)),
    "g16": _c((48, 0, 16, 3), F=49, M=4, offsets=(1, 16)),
    "g16_pad": _c((37, 0, 16, 3), F=38, M=4, offsets=(1, 16)),
    # with nsb = 3 no kept superblock has both neighbours: the sequential
    # two-product staging of k_cr_b (g >= 14) needs nsb >= 4
    "g13_nsb6": _c((71, 0, 13, 6), F=72, M=4, offsets=(1, 13)),
    "g14_nsb6": _c((71, 0, 14, 6), F=72, M=4, offsets=(1, 14)),
    "g16_nsb4": _c((59, 0, 16, 4), F=60, M=4, offsets=(1, 16)),
    # border sizes on a g = 2 chain: frame a is seen from two patches of a - 20
    "nB1": _c((38, 1, 2, 19), F=40, M=4, offsets=(1, 2), far=_border([30])),
    "nB16": _c((43, 16, 2, 22), F=60, M=4, offsets=(1, 2), far=_border(range(24, 56, 2))),
    "nB17": _c((42, 17, 2, 21), F=60, M=4, offsets=(1, 2), far=_border(range(24, 58, 2))),
    "nB64": _c((35, 64, 2, 18), F=100, M=3, offsets=(1, 2), far=_border(range(30, 94))),
    "nB65": _c((34, 65, 2, 17), "status", F=100, M=3, offsets=(1, 2),
               far=_border(range(30, 95))),
    # border assembly: a border pose inside a chain has later interior
    # neighbours; two border poses seen from one patch share a Cb block
    "border_then_interior": _c((22, 1, 2, 11), F=24, M=4, offsets=(1, 2), far=[(1, 19, 2)]),
    "border_pair": _c((37, 2, 1, 37), F=40, M=4, offsets=(1,), far=[(5, 30, 1), (5, 31, 1)]),
    # nB > 0 and more superblocks than border partial groups
    "border_many_sb": _c((37, 2, 1, 37), F=40, M=4, offsets=(1,),
                         far=[(5, 30, 2), (10, 36, 2)]),
    # the same on a graph with exactly nB17's E and N (same workspace size)
    "chain_like_nB17": _c((57, 2, 1, 57), F=60, M=8, offsets=(1,), seed=1,
                          far=[(5, 30, 2), (10, 36, 2)], extra={"dup": (0, 26)}),
    # one patch seen from exactly MAX_SET free poses, and from one more
    "set24": _c((24, 7, 16, 2), F=32, M=4, offsets=(1,),
                far=[(5, 5 + d, 1) for d in range(2, 24)]),
    "set25": _c((23, 8, 16, 2), "status", F=32, M=4, offsets=(1,),
                far=[(5, 5 + d, 1) for d in range(2, 25)]),
    # a free pose without any edge: the chain falls apart in two
    "isolated": _c((11, 0, 1, 11), F=12, M=4, offsets=(1,), extra={"isolate": 6}),
    "duplicates": _c((9, 0, 2, 5), F=10, M=4, offsets=(1, 2), extra={"dup": (10, 30)}),
    # fixed prefix: edges among fixed frames (patches without a free pose),
    # fixed -> free and free -> fixed edges; self edges (ii == jj) of a fixed
    # and of a free frame
    "fixed_prefix": _c((14, 0, 3, 5), t0=10, F=24, M=4, offsets=(1, 2, -1), far=[(12, 12, 2)],
                       extra={"fixed": [(2, 7, 3), (3, 3, 2)]}),
}

PARITY = [n for n, c in CASES.items() if c["kind"] == "parity"]

# every branch the table is there for (test_oracle_gba_cases checks that the
# union over the parity cases contains these, and which status case is which)
REQUIRED_BRANCHES = {
    "g1", "g2", "g5", "g13", "g14", "g16",
    "nsb1", "nsb2", "nsb3", "nsb4", "nsb5", "nsb6", "nsb7", "nsb9", "nsb>32",
    "nB0", "nB1", "nB16", "nB17", "nB64",
    "cr_b_both:two_fit", "cr_b_both:sequential", "cr_back_r:two_fit", "cr_back_r:sequential",
    "border_gj_regs", "border_gj_hbm", "no_border",
    "border_part_loop", "padded_last_superblock", "set24", "pose_without_block",
    "kept:-r-", "kept:-rR", "kept:lrR", "kept:lr-", "kept:l--", "elim:r", "elim:-",
    "asm_D", "asm_L", "asm_interior_above_border", "asm_border_above_interior",
    "asm_Cb_diag", "asm_Cb_off",
}


_graphs = {}


def graph(name):
    """The case's graph (built once per process; treat as read-only)."""
    if name not in _graphs:
        _graphs[name] = chain_graph(**CASES[name]["args"])
    return _graphs[name]


def case_structure(name):
    G, c = graph(name), CASES[name]
    return structure(G.ii.numpy(), G.jj.numpy(), G.kk.numpy(), c["t0"], G.F)
