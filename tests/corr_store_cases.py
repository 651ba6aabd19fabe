"""Inputs and case table of test_corr_store_paths_gpu.py and of
scripts/make_corr_store_golden.py (which records tests/golden/corr_store_parent.npz
at the commit before a change to how A-CORR stores its output blocks).

Everything is seeded numpy / CPU torch, so the recording and the test build the
same bits: one 17-edge set per shape, of which a case with E edges takes the
first E (an edge's block does not depend on the other edges, which the
recording asserts for every case before it keeps the 17-edge arrays only).
No GPU work at import, no test functions."""
import numpy as np
import torch

import corr_cases as C

E_MAX = 17
EDGE_COUNTS = (1, 2, 3, 9, 17)   # ordered: per = ceil(E / 8), eighths empty or of one edge;
                                 # 17: per = 3, half = 2, a pair across the half boundary
LEVEL_SETS = ((1, 2, 4, 8), (1, 2, 4), (1, 4), (1,))  # paired, paired odd L, unpaired 2 / 4 positions
DTYPES = {"f32": torch.float32, "f16": torch.float16}
H2, W2, N2, F, M_PATCH = 24, 32, 4, 4, 8
SEED = 2301


def graph():
    """The 17-edge patch graph whose reprojection gives coords and the XCD order."""
    from dpvo_amd import synthetic

    return synthetic.make_graph(F=F, M=M_PATCH, E=E_MAX, seed=SEED, H=H2, W=W2, p=3,
                                intr=(16.0, 16.0, 16.0, 12.0))


def features(levels, dtype, p=3, n1=F * M_PATCH):
    """gmap patches [1, n1, 128, p, p] and one independent random map per level
    [1, N2, 128, H2 / s, W2 / s], float32 arrays of values rounded to dtype."""
    r = np.random.default_rng(SEED + 10 * p)
    f1 = C.rounded(0.25 * r.standard_normal((1, n1, 128, p, p)), dtype)
    pyr = []
    for s in (1, 2, 4, 8):  # every level drawn, so a level's map does not depend on the set
        a = C.rounded(0.25 * r.standard_normal((1, N2, 128, H2 // s, W2 // s)), dtype)
        if s in levels:
            pyr.append(a)
    return f1, pyr


def dpvo_edges(dev, E, ordered, bad=False):
    """coords [1, E, 2, 3, 3], ii (gmap patch), jj (ring frame) of the first E edges and, if
    `ordered`, the order fastba.reproject(..., mem=) returns for them.  bad: edge 0's windows
    far outside every map (empty boxes on all levels), edge 2's ii out of range."""
    from dpvo_amd import fastba

    D = graph().to(dev)
    ii, jj, kk = D.ii[:E], D.jj[:E], D.kk[:E]
    if ordered:
        coords, order = fastba.reproject(D.poses, D.patches, D.intrinsics, ii, jj, kk, mem=N2)
    else:
        coords, order = fastba.reproject(D.poses, D.patches, D.intrinsics, ii, jj, kk), None
    coords, kk = coords.clone(), kk.clone()
    if bad:
        coords[:, 0] += 1.0e4
        if E > 2:
            kk[2] = F * M_PATCH + 3
    return coords, kk, jj % N2, order


def p2_edges():
    """The non-DPVO pair p = 2, R = 2 (run-time shape kernel): corr_cases._case inputs."""
    f1, f2, co, ii, jj, R = C._case(SEED + 1, M=E_MAX, N1=9, N2=N2, H2=H2, W2=W2, p=2, R=2, far=0.0)
    return co, ii, jj, R


def key(shape, dname, levels, bad=False):
    return f"{shape}{'_bad' if bad else ''}__{dname}__L{'_'.join(str(s) for s in levels)}"


def cases():
    """(id, dict(shape, dname, levels, E, ordered, bad))."""
    out = []
    for dname in DTYPES:
        for levels in LEVEL_SETS:
            for E in EDGE_COUNTS:
                for ordered in (False, True):
                    out.append(dict(shape="p3", dname=dname, levels=levels, E=E, ordered=ordered,
                                    bad=False))
        for levels in ((1, 2, 4, 8), (1, 4)):  # empty level-1 box, ii out of range
            for ordered in (False, True):
                out.append(dict(shape="p3", dname=dname, levels=levels, E=3, ordered=ordered,
                                bad=True))
        for levels in ((1, 2, 4, 8), (1, 4)):
            for ordered in (False, True):
                out.append(dict(shape="p2", dname=dname, levels=levels, E=E_MAX, ordered=ordered,
                                bad=False))
    return out


def case_id(c):
    return (f"{c['shape']}{'-bad' if c['bad'] else ''}-{c['dname']}-L{len(c['levels'])}-E{c['E']}"
            f"{'-ord' if c['ordered'] else ''}")


def run(dev, c):
    """One case on the GPU: (out [1, E, Dp, Dp, p, p, L] float32 tensor, again (the same call
    repeated into the same NaN-refilled block), reference inputs for the oracle)."""
    from dpvo_amd import altcorr, synthetic

    dtype, levels = DTYPES[c["dname"]], c["levels"]
    if c["shape"] == "p3":
        R, p = 3, 3
        f1, pyr = features(levels, dtype)
        coords, ii, jj, order = dpvo_edges(dev, c["E"], c["ordered"], c["bad"])
    else:
        co, ii_np, jj_np, R = p2_edges()
        p = 2
        f1, pyr = features(levels, dtype, p=2, n1=9)
        E = c["E"]
        coords, ii, jj = C._t(co[:, :E], dev), C._t(ii_np[:E], dev), C._t(jj_np[:E], dev)
        order = C._t(np.random.default_rng(SEED).permutation(E).astype(np.int32), dev) \
            if c["ordered"] else None
    g1 = C._t(f1, dev, dtype)
    lv = [synthetic.channels_last(C._t(a, dev, dtype)) for a in pyr]
    Dp = 2 * R + 1
    shape = (1, c["E"], Dp, Dp, p, p, len(levels))
    outs = []
    for _ in range(2):
        C.poison(shape, dev)  # the block torch::empty hands the extension next holds NaN
        out = altcorr.corr_levels(g1, lv, coords, ii, jj, R, scales=levels, order=order)
        torch.cuda.synchronize(dev)
        outs.append(out.view(shape).cpu().numpy())
        del out
    ref_in = (f1, pyr, coords.cpu().numpy(), ii.cpu().numpy(), jj.cpu().numpy(), R)
    return outs[0], outs[1], ref_in
