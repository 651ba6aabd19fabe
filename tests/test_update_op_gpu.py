"""GPU: the fused update operator (csrc/update_op.hip) against the fp64
restatement of tests/update_ref.py, which runs on the same device in float64.

Pass bars
  fp32 weights: max|got - ref| <= 1e-5 max|ref| for each of net_out, d, w (the
      project's fp32 bar of A-CORR).
  fp16 weights: the error of the restatement's f16_operand mode against fp64
      is computed on the same inputs; the GPU error must be <= 4 x that, per
      output (same rounding model, other summation order and rounding points).
  fp16 I/O: the restatement is fed the fp16-rounded inputs; rounding net_out
      adds 2^-11 max|ref|.
Every output is pre-filled with NaN and must be finite afterwards.
"""
import numpy as np
import pytest
import torch

from conftest import golden
import update_ref

pytestmark = pytest.mark.gpu
DIM = 384
WD = ["f32", "f16"]


class Ctx:
    def __init__(self, dev):
        import dpvo_amd

        self.dev = dev
        self.ext = dpvo_amd.load_extension("dpvo_update")
        self.params, self.blobs, self.ws, self.refs = {}, {}, {}, {}

    def P(self, key):
        """key: (K0, g_scale) -> (numpy fp32 params, fp64 device params)"""
        if key not in self.params:
            K0, gs = key
            p = update_ref.formula_params(K0)
            if gs != 1.0:
                for a in ("agg_kk", "agg_ij"):
                    p[a + ".g.weight"] = (p[a + ".g.weight"] * gs).astype(np.float32)
                    p[a + ".g.bias"] = (p[a + ".g.bias"] * gs).astype(np.float32)
            self.params[key] = (p, update_ref.to_torch(p, self.dev))
        return self.params[key]

    def blob(self, key, wd):
        """weights are packed and uploaded once per (parameters, dtype)"""
        if (key, wd) not in self.blobs:
            p = self.P(key)[0]
            ts = [torch.from_numpy(p[n]) for n, _ in update_ref.param_shapes(key[0])]
            code = self.ext.F16 if wd == "f16" else self.ext.F32
            self.blobs[(key, wd)] = (self.ext.pack_weights(ts, key[0], code).to(self.dev), code)
        return self.blobs[(key, wd)]

    def workspace(self, E, K0):
        n = self.ext.workspace_bytes(E, K0)
        if E not in self.ws:
            self.ws[E] = torch.empty(n, dtype=torch.uint8, device=self.dev)
        return self.ws[E]

    def run(self, key, wd, c, io=torch.float32, alias=False):
        E, K0 = c["net"].shape[0], key[0]
        blob, code = self.blob(key, wd)
        ws = self.workspace(E, K0)
        net = c["net"].to(io).clone()
        out = net if alias else torch.full_like(net, float("nan"))
        d = torch.full((E, 2), float("nan"), device=self.dev)
        w = torch.full((E, 2), float("nan"), device=self.dev)
        self.ext.plan(c["gk"], c["gij"], ws)
        self.ext.forward(blob, code, net, c["inp"].to(io), c["corr"].to(io), c["ix"], c["jx"], ws,
                         out, d, w)
        return out, d, w

    def ref(self, key, name, c, f16, io16=False):
        """fp64 restatement (and its f16_operand mode), computed once per case"""
        k = (key, name, f16, io16)
        if k not in self.refs:
            P = self.P(key)[1]
            r = (lambda t: t.half().double()) if io16 else (lambda t: t.double())
            self.refs[k] = update_ref.update_ref(P, r(c["net"]), r(c["inp"]), r(c["corr"]), c["ix"],
                                                 c["jx"], c["gk"], c["gij"], f16_operand=f16,
                                                 return_logits=True)
        return self.refs[k]


@pytest.fixture(scope="module")
def ctx(gpu):
    return Ctx(gpu)


def make_case(dev, E, K0, kind="dpvo", seed=0):
    ii, jj, kk = update_ref.dpvo_graph(E, M=8, seed=seed)
    if kind == "dup":  # duplicate (kk, jj) edges: every odd edge repeats its predecessor
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
    net, inp, corr = update_ref.inputs(E, K0, seed)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    return dict(net=t(net), inp=t(inp), corr=t(corr), ix=t(ix), jx=t(jx), gk=t(gk), gij=t(gij),
                ii=t(ii), jj=t(jj), kk=t(kk))


def err(got, ref):
    return float((got.double() - ref).abs().max())


def check(ctx, key, name, c, wd, io=torch.float32):
    io16 = io == torch.float16
    got = ctx.run(key, wd, c, io=io)
    ref = ctx.ref(key, name, c, False, io16)
    emu = ctx.ref(key, name, c, True, io16) if wd == "f16" else None
    ratios = {}
    for i, out in enumerate(("net_out", "d", "w")):
        assert torch.isfinite(got[i]).all(), out
        scale = float(ref[i].abs().max())
        e = err(got[i], ref[i])
        if wd == "f32":
            bound = 1e-5 * scale
        else:
            bound = 4.0 * err(emu[i], ref[i])
            if io16 and i == 0:
                bound += 2.0 ** -11 * scale
        ratios[out] = e / bound
        print(f"{name} {wd} {out}: err {e:.3e} = {e / scale:.3e} max|ref|, bound {bound:.3e}, "
              f"ratio {e / bound:.3f}")
    assert all(v <= 1.0 for v in ratios.values()), ratios
    return got, ref


@pytest.mark.parametrize("wd", WD)
def test_golden_case_through_the_forks_indices(ctx, wd):
    g = golden("update_fork_a")
    t = lambda a: torch.as_tensor(np.asarray(a)).to(ctx.dev)
    c = dict(net=t(g["net"]), inp=t(g["inp"]), corr=t(g["corr"]), ix=t(g["ix"]), jx=t(g["jx"]),
             gk=t(g["kk"]), gij=t(g["ii"]))
    got, _ = check(ctx, (882, 1.0), "golden", c, wd)
    if wd == "f32":  # and against the reference's own recorded output
        ref = t(g["net_out"])
        assert err(got[0], ref) <= 1e-5 * float(ref.abs().max())


# tile boundaries of the 16-row tile (E < 4096) and of the 32-row tile (from
# E = 4096): T - 1, T + 1, 2 T + 3 and full-tile counts, also for T = 64
SMALL_E = [1, 15, 16, 17, 31, 33, 35, 63, 64, 65, 67, 127, 129, 131, 257, 515]


@pytest.mark.parametrize("wd", WD)
@pytest.mark.parametrize("E", SMALL_E)
def test_edge_counts(ctx, E, wd):
    check(ctx, (882, 1.0), f"E{E}", make_case(ctx.dev, E, 882, seed=E), wd)


@pytest.mark.parametrize("wd", WD)
@pytest.mark.parametrize("E", [4096, 4097, 4159, 4227])
def test_edge_counts_large_tile(ctx, E, wd):
    # 4096 = 128 x 32; 4097 = +1; 4159 = 130 x 32 - 1; 4227 = 132 x 32 + 3
    check(ctx, (49, 1.0), f"L{E}", make_case(ctx.dev, E, 49, seed=E), wd)


@pytest.mark.parametrize("wd", WD)
@pytest.mark.parametrize("kind", ["dpvo", "one_group", "singletons", "no_neighbors", "reversed",
                                  "dup"])
def test_graph_shapes(ctx, kind, wd):
    check(ctx, (882, 1.0), "g_" + kind, make_case(ctx.dev, 200, 882, kind, seed=5), wd)


@pytest.mark.parametrize("wd", WD)
def test_large_logits_need_the_max_subtraction(ctx, wd):
    c = make_case(ctx.dev, 200, 882, seed=6)
    base = ctx.ref((882, 1.0), "logit_base", c, False)[3]
    key = (882, float(np.float32(80.0 / base)))
    ref = ctx.ref(key, "logit", c, False)
    assert 60.0 < ref[3] < 400.0, ref[3]  # exp(80) overflows fp32 without the subtraction
    check(ctx, key, "logit", c, wd)


@pytest.mark.parametrize("wd", WD)
def test_out_of_range_indices_are_missing_neighbours(ctx, wd):
    c = make_case(ctx.dev, 200, 882, seed=7)
    assert (c["ix"] < 0).any() and (c["jx"] < 0).any()
    want = ctx.run((882, 1.0), wd, c)
    E = 200
    c2 = dict(c)
    c2["ix"] = torch.where(c["ix"] < 0, torch.full_like(c["ix"], -7), c["ix"])
    c2["jx"] = torch.where(c["jx"] < 0, torch.full_like(c["jx"], E + 5), c["jx"])
    got = check(ctx, (882, 1.0), "oob", c2, wd)[0]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    c3 = dict(c, ix=c2["jx"].clone(), jx=torch.full_like(c["jx"], E))  # E itself is outside
    c3ref = dict(c, ix=torch.where(c2["jx"] >= E, -1, c2["jx"]), jx=torch.full_like(c["jx"], -1))
    for a, b in zip(ctx.run((882, 1.0), wd, c3), ctx.run((882, 1.0), wd, c3ref)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("wd", WD)
def test_one_level_corr_dim_49(ctx, wd):
    check(ctx, (49, 1.0), "k49", make_case(ctx.dev, 200, 49, seed=8), wd)


@pytest.mark.parametrize("wd", WD)
@pytest.mark.parametrize("E", [2048, 9850])
def test_live_sizes(ctx, E, wd):
    check(ctx, (882, 1.0), f"S{E}", make_case(ctx.dev, E, 882, seed=9), wd)


@pytest.mark.parametrize("E", [200, 4159])
def test_fp16_io(ctx, E):
    K0 = 882 if E == 200 else 49
    got, _ = check(ctx, (K0, 1.0), f"io16_{E}", make_case(ctx.dev, E, K0, seed=10), "f16",
                   io=torch.float16)
    assert got[0].dtype == torch.float16 and got[1].dtype == torch.float32


@pytest.mark.parametrize("wd", WD)
@pytest.mark.parametrize("E", [200, 4159])
def test_repeatable_and_alias(ctx, E, wd):
    K0 = 882 if E == 200 else 49
    c = make_case(ctx.dev, E, K0, seed=11)
    a = ctx.run((K0, 1.0), wd, c)
    b = ctx.run((K0, 1.0), wd, c)
    al = ctx.run((K0, 1.0), wd, c, alias=True)
    for x, y, z in zip(a, b, al):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("wd", WD)
def test_graph_replay_is_bit_identical(ctx, wd):
    E, K0 = 257, 882
    c = make_case(ctx.dev, E, K0, seed=12)
    eager = ctx.run((K0, 1.0), wd, c)  # also the warm-up (one-time kernel attributes)
    blob, code = ctx.blob((K0, 1.0), wd)
    ws = ctx.workspace(E, K0)
    out = torch.full((E, DIM), float("nan"), device=ctx.dev)
    d, w = torch.full((E, 2), float("nan"), device=ctx.dev), torch.full((E, 2), float("nan"),
                                                                          device=ctx.dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.ext.plan(c["gk"], c["gij"], ws)
        ctx.ext.forward(blob, code, c["net"], c["inp"], c["corr"], c["ix"], c["jx"], ws, out, d, w)
    for _ in range(2):
        out.fill_(float("nan")), d.fill_(float("nan")), w.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip((out, d, w), eager):
            assert torch.equal(x, y)


@pytest.mark.parametrize("wd", WD)
def test_module_matches_raw_call_and_default_indices(ctx, wd):
    from dpvo_amd import fastba
    from dpvo_amd.net import Update

    E, K0 = 200, 882
    c = make_case(ctx.dev, E, K0, seed=13)
    dt = torch.float16 if wd == "f16" else torch.float32
    m = Update(p=3, dtype=dt)
    sd = {k: torch.from_numpy(v) for k, v in ctx.P((K0, 1.0))[0].items()}
    assert list(m.state_dict()) == [n for n, _ in update_ref.param_shapes(K0)]
    m.load_state_dict(sd)
    ix, jx = fastba.neighbors(c["kk"], c["jj"])
    assert torch.equal(ix.long(), c["ix"]) and torch.equal(jx.long(), c["jx"])
    raw = ctx.run((K0, 1.0), wd, c)  # explicit neighbours, kk, ii * 12345 + jj
    net, (d, w, none) = m(c["net"][None], c["inp"][None], c["corr"][None], None, c["ii"], c["jj"],
                          c["kk"])
    assert none is None and net.shape == (1, E, DIM) and d.shape == w.shape == (1, E, 2)
    assert torch.equal(net[0], raw[0]) and torch.equal(d[0], raw[1]) and torch.equal(w[0], raw[2])
    # explicit indices: the fork's variant (groups kk and ii)
    cf = dict(c, gij=c["ii"])
    rawf = ctx.run((K0, 1.0), wd, cf)
    netf, (df, wf, _) = m(c["net"][None], c["inp"][None], c["corr"][None], None, c["ii"], c["jj"],
                          c["kk"], ix=c["ix"], jx=c["jx"], gk=c["kk"], gij=c["ii"])
    assert torch.equal(netf[0], rawf[0]) and torch.equal(df[0], rawf[1])
    assert not torch.equal(netf, net)
    # from_reference copies; a parameter write repacks
    m2 = Update.from_reference(m, dtype=dt)
    net2 = m2(c["net"][None], c["inp"][None], c["corr"][None], None, c["ii"], c["jj"], c["kk"])[0]
    assert torch.equal(net2, net)
    with torch.no_grad():
        m2.norm.bias.add_(0.25)
    net3 = m2(c["net"][None], c["inp"][None], c["corr"][None], None, c["ii"], c["jj"], c["kk"])[0]
    assert not torch.equal(net3, net)
