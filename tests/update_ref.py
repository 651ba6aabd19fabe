"""fp64 restatement of DPVO's update operator, written from its formulas:

    t  = relu(corr Wc0^T + b);  t = relu(LN(t Wc2^T + b));  t = t Wc5^T + b
    x  = LN(net + inp + t)
    x += c1(m_ix * x[ix]);  x += c2(m_jx * x[jx])      c = Linear, ReLU, Linear
    x += h(sum_group softmax_group(g(x)) * f(x))[group of e]      groups gk, then gij
    x  = GatedResidual(LN(x)) twice                     x + sigmoid(gate x) * res(x)
    d  = Wd relu(x) + b;  w = sigmoid(Ww relu(x) + b)

LayerNorm has eps 1e-3; an index outside [0, E) is a missing neighbour (mask
0).  Runs on whatever device its inputs are on, in float64.  With
``f16_operand=True`` the input and the weight of every linear are rounded to
fp16 (nearest even) and nothing else changes: the rounding model of the fp16
kernels.
"""
import math

import numpy as np
import torch

DIM = 384

# (name, shape builder) in the state_dict order of the reference's Update
def param_shapes(K0):
    lin = lambda n, o, i: [(n + ".weight", (o, i)), (n + ".bias", (o,))]
    ln = lambda n: [(n + ".weight", (DIM,)), (n + ".bias", (DIM,))]
    out = []
    for c in ("c1", "c2"):
        out += lin(c + ".0", DIM, DIM) + lin(c + ".2", DIM, DIM)
    out += ln("norm")
    for a in ("agg_kk", "agg_ij"):
        for s in "fgh":
            out += lin(f"{a}.{s}", DIM, DIM)
    for n, g in (("gru.0", "gru.1"), ("gru.2", "gru.3")):
        out += ln(n) + lin(g + ".gate.0", DIM, DIM) + lin(g + ".res.0", DIM, DIM)
        out += lin(g + ".res.2", DIM, DIM)
    out += lin("corr.0", DIM, K0) + lin("corr.2", DIM, DIM) + ln("corr.3") + lin("corr.5", DIM, DIM)
    out += lin("d.1", 2, DIM) + lin("w.1", 2, DIM)
    return out


def _hash01(idx, salt):
    """Closed-form pseudo-noise in [-1, 1): the fractional part of a scaled sine."""
    v = np.sin(idx * 12.9898 + salt * 78.233 + 0.5) * 43758.5453
    return 2.0 * (v - np.floor(v)) - 1.0


def formula_params(K0):
    """Deterministic parameters from a closed formula (no RNG), as float32
    numpy arrays keyed by state_dict name.  Linear weights are uniform-like
    with standard deviation 1 / sqrt(fan_in); LayerNorm gains sit in
    [0.7, 1.3] and every bias is away from 0."""
    out = {}
    for t, (name, shape) in enumerate(param_shapes(K0)):
        n = int(np.prod(shape))
        u = _hash01(np.arange(n, dtype=np.float64), t + 1).reshape(shape)
        leaf = name.split(".")
        is_ln = name.startswith("norm") or name in ("gru.0.weight", "gru.0.bias", "gru.2.weight",
                                                     "gru.2.bias", "corr.3.weight", "corr.3.bias")
        if is_ln:
            v = 1.0 + 0.3 * u if leaf[-1] == "weight" else 0.2 * u + 0.05
        elif leaf[-1] == "weight":
            v = u * math.sqrt(3.0 / shape[1])
        else:
            v = 0.1 * u + 0.02
        out[name] = v.astype(np.float32)
    return out


def to_torch(params, device="cpu"):
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float64, device=device)
            for k, v in params.items()}


def _r16(t):
    return t.to(torch.float16).to(torch.float64)


def _ln(P, name, x):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-3) * P[name + ".weight"] + P[name + ".bias"]


def update_ref(P, net, inp, corr, ix, jx, gk, gij, f16_operand=False, return_logits=False):
    """P: dict of float64 tensors (to_torch).  net, inp [E, 384], corr [E, K0]
    float64; ix, jx, gk, gij integer [E].  Returns net_out [E, 384], d, w
    [E, 2] (and max |g| over both aggregations with return_logits)."""
    E = net.shape[0]

    def lin(name, x):
        W = P[name + ".weight"]
        if f16_operand:
            x, W = _r16(x), _r16(W)
        return x @ W.T + P[name + ".bias"]

    def gather(x, idx):
        idx = idx.long()
        ok = (idx >= 0) & (idx < E)
        return x[idx.clamp(0, E - 1)] * ok.to(x.dtype)[:, None]

    logit = [0.0]

    def agg(name, x, ids):
        _, inv = torch.unique(ids.long(), return_inverse=True)
        G = int(inv.max()) + 1
        f, g = lin(name + ".f", x), lin(name + ".g", x)
        logit[0] = max(logit[0], float(g.abs().max()))
        col = inv[:, None].expand(-1, DIM)
        gmax = torch.full((G, DIM), -math.inf, dtype=x.dtype, device=x.device)
        gmax = gmax.scatter_reduce(0, col, g, "amax", include_self=True)
        ex = torch.exp(g - gmax[inv])
        den = torch.zeros((G, DIM), dtype=x.dtype, device=x.device).index_add_(0, inv, ex)
        y = torch.zeros((G, DIM), dtype=x.dtype, device=x.device).index_add_(0, inv, f * ex / den[inv])
        return lin(name + ".h", y)[inv]

    t = torch.relu(lin("corr.0", corr))
    t = torch.relu(_ln(P, "corr.3", lin("corr.2", t)))
    t = lin("corr.5", t)
    x = _ln(P, "norm", net + inp + t)
    x = x + lin("c1.2", torch.relu(lin("c1.0", gather(x, ix))))
    x = x + lin("c2.2", torch.relu(lin("c2.0", gather(x, jx))))
    x = x + agg("agg_kk", x, gk)
    x = x + agg("agg_ij", x, gij)
    for n, g in (("gru.0", "gru.1"), ("gru.2", "gru.3")):
        x = _ln(P, n, x)
        x = x + torch.sigmoid(lin(g + ".gate.0", x)) * lin(g + ".res.2",
                                                           torch.relu(lin(g + ".res.0", x)))
    d = lin("d.1", torch.relu(x))
    w = torch.sigmoid(lin("w.1", torch.relu(x)))
    if return_logits:
        return x, d, w, logit[0]
    return x, d, w


def neighbors_ref(kk, jj):
    """fastba.neighbors restated (ba.cpp:59-97): previous / next edge of the
    same kk ordered by jj (stable), -1 at the ends.  numpy int64."""
    kk, jj = np.asarray(kk), np.asarray(jj)
    E = len(kk)
    ix, jx = np.full(E, -1, np.int64), np.full(E, -1, np.int64)
    order = np.lexsort((np.arange(E), jj, kk))
    for a, b in zip(order[:-1], order[1:]):
        if kk[a] == kk[b]:
            jx[a], ix[b] = b, a
    return ix, jx


def dpvo_graph(E, M=8, seed=0, min_deg=1, max_deg=10):
    """A DPVO-shaped edge list: patch k of frame k // M is seen in 1-10 target
    frames.  Returns int64 ii, jj, kk of exactly E edges in shuffled order."""
    rng = np.random.RandomState(seed)
    ii, jj, kk = [], [], []
    k = 0
    while len(kk) < E:
        i = k // M
        cand = np.arange(max(0, i - 6), i + 7)
        deg = min(rng.randint(min_deg, max_deg + 1), len(cand))
        for j in rng.choice(cand, size=deg, replace=False):
            ii.append(i), jj.append(int(j)), kk.append(k)
        k += 1
    perm = rng.permutation(len(kk))[:E]
    f = lambda a: np.asarray(a, np.int64)[perm]
    return f(ii), f(jj), f(kk)


def inputs(E, K0, seed=0):
    """fp32-representable net, inp, corr as float32 numpy arrays."""
    rng = np.random.RandomState(1000 + seed)
    return ((0.5 * rng.randn(E, DIM)).astype(np.float32), (0.5 * rng.randn(E, DIM)).astype(np.float32),
            rng.randn(E, K0).astype(np.float32))
