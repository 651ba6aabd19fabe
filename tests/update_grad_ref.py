"""The yardstick of the update operator's backward: tests/update_ref.py restated
with injectable ReLU masks, the case list, and the bars.

Why masks are injected.  A ReLU's mask is a step function of its
pre-activation p.  An fp32 forward and the fp64 restatement disagree on it
wherever p is within rounding of zero, and one flipped entry changes the
gradient by percents (fp32 against fp64 autograd of update_ref itself: 7e-2 of
max|ref| at E = 200, seed 0).  So every ReLU here is ``p * mask``; ``mask``
defaults to ``p > 0`` and can be given per ReLU.  The GPU test reads the masks
the device used, injects them, and compares the kernels with the exact
gradient of the function they evaluated.  A second check keeps the masks
honest: a device mask may differ from ``p > 0`` only where |p| <= tau with
tau = 1e-5 max|p| of that ReLU's plane (1e-5 max|ref| is the forward's own fp32
bar), and the share of such positions, computed from fp64 alone, is at most
NEAR_TIE_CAP in every case, so the comparison is never empty.

The softmax maximum is detached (it cancels analytically).  With default masks
the fp64 outputs equal update_ref.update_ref exactly.
"""
import math

import numpy as np
import torch

import update_ref

DIM = 384
# the seven ReLUs, in the order of the device's mask read-out; the last one
# (the heads' relu(x)) is net_out > 0
RELUS = ("corr.0", "corr.3", "c1.0", "c2.0", "gru.1.res.0", "gru.3.res.0", "heads")
TAU_REL = 1e-5
NEAR_TIE_CAP = 2e-4

# (E, K0, kind, seed)
CASES = [(1, 49, "dpvo", 0), (15, 49, "dpvo", 0), (16, 882, "dpvo", 16), (17, 882, "dpvo", 0),
         (33, 882, "dpvo", 0), (200, 882, "dpvo", 0), (200, 882, "dpvo", 1), (4097, 49, "dpvo", 4097),
         (200, 882, "dpvo", 5), (200, 882, "one_group", 5), (200, 882, "singletons", 5),
         (200, 882, "no_neighbors", 5), (200, 882, "reversed", 5), (200, 882, "dup", 5),
         (200, 882, "fan_in", 5)]


def case_id(c):
    return f"E{c[0]}-K{c[1]}-{c[2]}-s{c[3]}"


def make_case(dev, E, K0, kind="dpvo", seed=0):
    """The graph shapes of test_update_op_gpu.make_case, restated, plus
    ``fan_in``: ix = e // 4 and jx = 0, so four edges scatter into one row and
    all of them into row 0."""
    ii, jj, kk = update_ref.dpvo_graph(E, M=8, seed=seed)
    if kind == "dup":  # every odd edge repeats its predecessor
        n = E // 2
        for a in (ii, jj, kk):
            a[1:2 * n:2] = a[0:2 * n:2]
    ix, jx = update_ref.neighbors_ref(kk, jj)
    gk, gij = kk.copy(), ii * 12345 + jj
    if kind == "one_group":
        gk[:], gij[:] = 7, -3
    elif kind == "singletons":
        gk, gij = np.arange(E)[::-1] * 5 - 100, np.arange(E) * (1 << 33)
    elif kind == "no_neighbors":
        ix[:], jx[:] = -1, -1
    elif kind == "reversed":
        ix, jx = np.arange(E)[::-1].copy(), (np.arange(E) * 37 + 11) % E
    elif kind == "fan_in":
        ix, jx = np.arange(E) // 4, np.zeros(E, np.int64)
    net, inp, corr = update_ref.inputs(E, K0, seed)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    return dict(net=t(net), inp=t(inp), corr=t(corr), ix=t(ix).long(), jx=t(jx).long(),
                gk=t(gk).long(), gij=t(gij).long(), ii=t(ii), jj=t(jj), kk=t(kk))


def cotangents(E, seed, dev):
    """fp32-representable cotangents of net_out, d, w, as float64."""
    rng = np.random.RandomState(5000 + seed)
    f = lambda *s: torch.as_tensor(rng.randn(*s).astype(np.float32), device=dev).double()
    return f(E, DIM), f(E, 2), f(E, 2)


def _ln(P, name, x):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-3) * P[name + ".weight"] + P[name + ".bias"]


def update_masked(P, net, inp, corr, ix, jx, gk, gij, masks=None, pre=None):
    """update_ref.update_ref (no f16 mode) in the dtype of its inputs, every
    ReLU as p * mask.  masks: {name of RELUS: bool tensor}; a missing name
    means p > 0.  pre: a dict that receives every ReLU's detached
    pre-activation.  Returns net_out, d, w."""
    E = net.shape[0]
    masks = masks or {}

    def lin(name, x):
        return x @ P[name + ".weight"].T + P[name + ".bias"]

    def relu(name, p):
        if pre is not None:
            pre[name] = p.detach()
        m = masks.get(name)
        m = (p > 0) if m is None else m.to(torch.bool)
        return torch.where(m, p, torch.zeros((), dtype=p.dtype, device=p.device))

    def gather(x, idx):
        idx = idx.long()
        ok = (idx >= 0) & (idx < E)
        return x[idx.clamp(0, E - 1)] * ok.to(x.dtype)[:, None]

    def agg(name, x, ids):
        _, inv = torch.unique(ids.long(), return_inverse=True)
        G = int(inv.max()) + 1
        f, g = lin(name + ".f", x), lin(name + ".g", x)
        col = inv[:, None].expand(-1, DIM)
        gmax = torch.full((G, DIM), -math.inf, dtype=x.dtype, device=x.device)
        gmax = gmax.scatter_reduce(0, col, g.detach(), "amax", include_self=True)
        ex = torch.exp(g - gmax[inv])
        den = torch.zeros((G, DIM), dtype=x.dtype, device=x.device).index_add_(0, inv, ex)
        y = torch.zeros((G, DIM), dtype=x.dtype, device=x.device).index_add_(0, inv, f * ex / den[inv])
        return lin(name + ".h", y)[inv]

    t = relu("corr.0", lin("corr.0", corr))
    t = relu("corr.3", _ln(P, "corr.3", lin("corr.2", t)))
    t = lin("corr.5", t)
    x = _ln(P, "norm", net + inp + t)
    x = x + lin("c1.2", relu("c1.0", lin("c1.0", gather(x, ix))))
    x = x + lin("c2.2", relu("c2.0", lin("c2.0", gather(x, jx))))
    x = x + agg("agg_kk", x, gk)
    x = x + agg("agg_ij", x, gij)
    for n, g in (("gru.0", "gru.1"), ("gru.2", "gru.3")):
        x = _ln(P, n, x)
        x = x + torch.sigmoid(lin(g + ".gate.0", x)) * lin(g + ".res.2",
                                                           relu(g + ".res.0", lin(g + ".res.0", x)))
    r = relu("heads", x)
    d = lin("d.1", r)
    w = torch.sigmoid(lin("w.1", r))
    return x, d, w


def names(K0):
    return [n for n, _ in update_ref.param_shapes(K0)]


def grads(P, c, cot, masks=None, dtype=torch.float64):
    """Autograd of sum(out * cot) through update_masked in `dtype`: the
    gradients of net, inp, corr and of the 50 parameters (state_dict order),
    as float64.  P: float64 parameter dict; c: a case; cot: float64."""
    K0 = c["corr"].shape[1]
    Pd = {k: v.detach().to(dtype).requires_grad_() for k, v in P.items()}
    x = [c[k].detach().to(dtype).clone().requires_grad_() for k in ("net", "inp", "corr")]
    out = update_masked(Pd, x[0], x[1], x[2], c["ix"], c["jx"], c["gk"], c["gij"], masks=masks)
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(out, cot))
    g = torch.autograd.grad(loss, x + [Pd[k] for k in names(K0)])
    return [t.double() for t in g]


def near_tie_share(pre):
    """Share of ReLU positions with |p| <= TAU_REL max|p| of their plane."""
    n = sum(p.numel() for p in pre.values())
    k = sum(int((p.abs() <= TAU_REL * float(p.abs().max())).sum()) for p in pre.values())
    return k / n


def structural_zero(name, kind):
    """Tensors whose exact gradient is zero in a case of this kind."""
    if name in ("agg_kk.g.bias", "agg_ij.g.bias"):
        return True
    if kind == "singletons" and name in ("agg_kk.g.weight", "agg_ij.g.weight"):
        return True
    return kind == "no_neighbors" and name in ("c1.0.weight", "c2.0.weight")
