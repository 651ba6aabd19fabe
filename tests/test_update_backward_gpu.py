"""GPU: the update operator's training forward, HIP backward and autograd
plumbing (csrc/update_op.hip, csrc/update_bwd.hip, dpvo_amd.net.Update with
differentiable=True) against fp64 autograd of the mask-injected restatement
(tests/update_grad_ref.py) on the same device.

Bar per gradient tensor (net, inp, corr and the 50 parameters):
    max|got - ref| <= max(1e-5 max|ref|, 4 err32)
where ref is the fp64 autograd of the restatement with the device's own seven
ReLU masks injected and err32 is the error of fp32 PyTorch autograd of the same
mask-injected restatement against ref.  1e-5 is the project's fp32 bar; 4 is
the margin the forward's fp16 test gives over its emulation.  A parameter
tensor whose max|ref| is below 1e-9 of the largest max|ref| among the 50
parameter gradients of the case is a structural zero (agg_*.g.bias always;
agg_*.g.weight with singleton groups; c1.0 / c2.0 weights without neighbours)
and is held to 1e-5 times that largest maximum.

The device masks may differ from the fp64 masks p > 0 only where |p| <= 1e-5
max|p| of that ReLU's plane.

Every gradient buffer is pre-filled with NaN and must be finite afterwards.
"""
import numpy as np
import pytest
import torch

import update_grad_ref as ugr
import update_ref

pytestmark = pytest.mark.gpu
DIM = 384
LOGIT_CASE = (200, 882, "dpvo", 6)  # the sixteenth case: agg_*.g scaled to max|g| in (60, 400)


class Ctx:
    def __init__(self, dev):
        import dpvo_amd

        self.dev = dev
        self.ext = dpvo_amd.load_extension("dpvo_update")
        self.params, self.cases, self.full = {}, {}, {}

    def P(self, key):
        """key: (K0, g_scale) -> (fp32 device tensors in state_dict order, fp64 device dict)"""
        if key not in self.params:
            K0, gs = key
            p = update_ref.formula_params(K0)
            if gs != 1.0:
                for a in ("agg_kk", "agg_ij"):
                    p[a + ".g.weight"] = (p[a + ".g.weight"] * gs).astype(np.float32)
                    p[a + ".g.bias"] = (p[a + ".g.bias"] * gs).astype(np.float32)
            ts = [torch.from_numpy(p[n]).to(self.dev) for n in ugr.names(K0)]
            self.params[key] = (ts, update_ref.to_torch(p, self.dev))
        return self.params[key]

    def case(self, c):
        if c not in self.cases:
            self.cases[c] = ugr.make_case(self.dev, *c)
        return self.cases[c]

    def forward(self, key, c):
        """pack_weights_device + plan + forward_train -> ((net_out, d, w), saved)"""
        x, K0 = self.ext, key[0]
        E = c["net"].shape[0]
        ts = self.P(key)[0]
        blob = torch.empty(x.packed_bytes(K0, x.F32), dtype=torch.uint8, device=self.dev)
        x.pack_weights_device(ts, K0, x.F32, blob)
        ws = torch.empty(x.workspace_bytes(E, K0), dtype=torch.uint8, device=self.dev)
        saved = torch.empty(x.saved_bytes(E, K0), dtype=torch.uint8, device=self.dev)
        out = [torch.full((E, n), float("nan"), device=self.dev) for n in (DIM, 2, 2)]
        x.plan(c["gk"], c["gij"], ws)
        x.forward_train(blob, c["net"], c["inp"], c["corr"], c["ix"], c["jx"], ws, saved, *out)
        return out, saved

    def backward(self, key, c, saved, cot, want=(True, True, True), params=True):
        """-> [g_net, g_inp, g_corr] (None where not wanted) + the 50 parameter gradients"""
        x, K0 = self.ext, key[0]
        E = c["net"].shape[0]
        ts = self.P(key)[0]
        gin = [torch.full((E, n), float("nan"), device=self.dev) if w else None
               for n, w in zip((DIM, DIM, K0), want)]
        grads = [torch.full_like(t, float("nan")) for t in ts] if params else []
        ws = torch.full((x.backward_workspace_bytes(E, K0),), 0xFF, dtype=torch.uint8,
                        device=self.dev)
        x.backward(ts, saved, c["ix"], c["jx"], K0, cot[0], cot[1], cot[2], gin[0], gin[1], gin[2],
                   grads, ws)
        for g in gin + grads:
            assert g is None or torch.isfinite(g).all(), "not fully written"
        return gin + grads

    def everything(self, case, key=None):
        """Once per case: the device run, its masks, the fp64 pre-activations,
        the mask-injected fp64 reference and the fp32 autograd's error."""
        key = key or (case[1], 1.0)
        k = (case, key)
        if k in self.full:
            return self.full[k]
        c = self.case(case)
        E, K0 = case[0], case[1]
        P64 = self.P(key)[1]
        out, saved = self.forward(key, c)
        m = self.ext.relu_masks(saved, E, K0)
        masks = {n: m[i].bool() for i, n in enumerate(ugr.RELUS[:6])}
        masks["heads"] = out[0] > 0
        pre = {}
        with torch.no_grad():
            ref_out = ugr.update_masked(P64, c["net"].double(), c["inp"].double(),
                                        c["corr"].double(), c["ix"], c["jx"], c["gk"], c["gij"],
                                        pre=pre)
        cot = ugr.cotangents(E, case[3], self.dev)
        ref = ugr.grads(P64, c, cot, masks=masks)
        g32 = ugr.grads(P64, c, cot, masks=masks, dtype=torch.float32)
        got = self.backward(key, c, saved, [t.float() for t in cot])
        self.full[k] = dict(c=c, out=out, saved=saved, masks=masks, pre=pre, ref_out=ref_out,
                            cot=cot, ref=ref, g32=g32, got=got)
        return self.full[k]


@pytest.fixture(scope="module")
def ctx(gpu):
    return Ctx(gpu)


def family(name):
    if name in ("net", "inp", "corr"):
        return "inputs"
    if name.startswith(("d.1", "w.1")):
        return "heads"
    if name.startswith(("norm", "gru.0", "gru.2", "corr.3")):
        return "layernorm"
    return "weights" if name.endswith("weight") else "biases"


def check_grads(got, ref, g32, K0, label):
    """The bar on each of the 53 tensors; prints the worst ratio err / bound per family."""
    names = ["net", "inp", "corr"] + ugr.names(K0)
    pmax = max(float(r.abs().max()) for r in ref[3:])
    worst, bad = {}, []
    for name, g, r, g3 in zip(names, got, ref, g32):
        assert g.shape == r.shape, name
        err, scale = float((g.double() - r).abs().max()), float(r.abs().max())
        err32 = float((g3 - r).abs().max())
        if name not in names[:3] and scale < 1e-9 * pmax:
            fam, bound = "structural zeros", 1e-5 * pmax
        else:
            fam, bound = family(name), max(1e-5 * scale, 4.0 * err32)
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if ratio >= worst.get(fam, (-1.0, ""))[0]:
            worst[fam] = (ratio, name)
        if not ratio <= 1.0:
            bad.append((name, err, scale, err32))
    print(f"PARITY update_bwd {label} " +
          ", ".join(f"{f} {v[0]:.3f} ({v[1]})" for f, v in sorted(worst.items())) +
          " (err / bound, bar 1)")
    assert not bad, bad
    return worst


def check_masks(r):
    for name in ugr.RELUS:
        p, m = r["pre"][name], r["masks"][name]
        flips = m != (p > 0)
        tau = ugr.TAU_REL * float(p.abs().max())
        n = int(flips.sum())
        worst = float(p[flips].abs().max()) if n else 0.0
        print(f"MASKS {name}: {n} of {p.numel()} differ, largest |p| {worst:.3e}, tau {tau:.3e}")
        assert worst <= tau, name


@pytest.mark.parametrize("case", ugr.CASES, ids=ugr.case_id)
def test_gradients_match_autograd_of_the_mask_injected_restatement(ctx, case):
    r = ctx.everything(case)
    for got, ref in zip(r["out"], r["ref_out"]):  # the forward's own bar
        assert float((got.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    check_grads(r["got"], r["ref"], r["g32"], case[1], ugr.case_id(case))


@pytest.mark.parametrize("case", ugr.CASES, ids=ugr.case_id)
def test_device_masks_equal_the_fp64_masks_outside_the_band(ctx, case):
    check_masks(ctx.everything(case))


def test_structural_zeros_are_where_they_are_expected(ctx):
    for case in [c for c in ugr.CASES if c[0] == 200 and c[3] == 5]:
        r = ctx.everything(case)
        names = ugr.names(case[1])
        pmax = max(float(t.abs().max()) for t in r["ref"][3:])
        zeros = {n for n, t in zip(names, r["ref"][3:]) if float(t.abs().max()) < 1e-9 * pmax}
        assert zeros == {n for n in names if ugr.structural_zero(n, case[2])}, case


@pytest.mark.parametrize("E", [17, 200, 4097, 4159])
def test_training_forward_equals_inference_forward(ctx, E):
    K0 = 882 if E <= 200 else 49
    key = (K0, 1.0)
    c = ugr.make_case(ctx.dev, E, K0, seed=E)
    x = ctx.ext
    host = x.pack_weights([t.cpu() for t in ctx.P(key)[0]], K0, x.F32).to(ctx.dev)
    ws = torch.empty(x.workspace_bytes(E, K0), dtype=torch.uint8, device=ctx.dev)
    inf = [torch.full((E, n), float("nan"), device=ctx.dev) for n in (DIM, 2, 2)]
    x.plan(c["gk"], c["gij"], ws)
    x.forward(host, x.F32, c["net"], c["inp"], c["corr"], c["ix"], c["jx"], ws, *inf)
    out, _ = ctx.forward(key, c)
    for a, b in zip(out, inf):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_null_cotangents_are_zeros_and_unwanted_gradients_change_nothing(ctx):
    case = (200, 882, "dpvo", 5)
    r = ctx.everything(case)
    key, c, saved = (882, 1.0), r["c"], r["saved"]
    cot = [t.float() for t in r["cot"]]
    for null in range(3):
        z = [torch.zeros_like(t) if i == null else t for i, t in enumerate(cot)]
        n = [None if i == null else t for i, t in enumerate(cot)]
        for a, b in zip(ctx.backward(key, c, saved, z), ctx.backward(key, c, saved, n)):
            assert torch.equal(a, b)
    for want in [(False, True, True), (True, False, False), (False, False, False)]:
        got = ctx.backward(key, c, saved, cot, want=want)
        for w, a, b in zip(want + (True,) * 50, got, r["got"]):
            assert (a is None) if not w else torch.equal(a, b)
    only_inputs = ctx.backward(key, c, saved, cot, params=False)
    assert len(only_inputs) == 3
    for a, b in zip(only_inputs, r["got"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["fan_in", "one_group"])
def test_two_runs_are_bit_identical(ctx, kind):
    case = (200, 882, kind, 5)
    r = ctx.everything(case)
    out, saved = ctx.forward((882, 1.0), r["c"])
    again = ctx.backward((882, 1.0), r["c"], saved, [t.float() for t in r["cot"]])
    for a, b in zip(again, r["got"]):
        assert torch.equal(a, b)


def test_a_second_forward_with_another_E_leaves_the_first_backward_alone(ctx):
    """The group plans the backward needs live in `saved`, not in the shared workspace."""
    x, key = ctx.ext, (882, 1.0)
    r = ctx.everything((200, 882, "dpvo", 5))
    c1, c2 = r["c"], ctx.case((33, 882, "dpvo", 0))
    ts = ctx.P(key)[0]
    blob = torch.empty(x.packed_bytes(882, x.F32), dtype=torch.uint8, device=ctx.dev)
    x.pack_weights_device(ts, 882, x.F32, blob)
    ws = torch.empty(x.workspace_bytes(200, 882), dtype=torch.uint8, device=ctx.dev)  # shared
    saved = []
    for c in (c1, c2):
        E = c["net"].shape[0]
        s = torch.empty(x.saved_bytes(E, 882), dtype=torch.uint8, device=ctx.dev)
        out = [torch.empty(E, n, device=ctx.dev) for n in (DIM, 2, 2)]
        x.plan(c["gk"], c["gij"], ws)
        x.forward_train(blob, c["net"], c["inp"], c["corr"], c["ix"], c["jx"], ws, s, *out)
        saved.append(s)
    ws.fill_(0xFF)
    got = ctx.backward(key, c1, saved[0], [t.float() for t in r["cot"]])
    for a, b in zip(got, r["got"]):
        assert torch.equal(a, b)


def module(ctx, K0=882, differentiable=True, vonet=False):
    from dpvo_amd.net import Update, VONet

    if vonet:
        m = VONet(dtype=torch.float32, differentiable=differentiable).update
        assert m.differentiable == differentiable
    else:
        m = Update(p=3, dtype=torch.float32, corr_dim=K0, differentiable=differentiable)
    p = update_ref.formula_params(K0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return m.to(ctx.dev)


def call(m, c, req=True):
    x = [c[k].detach()[None].clone().requires_grad_(req) for k in ("net", "inp", "corr")]
    net, (d, w, none) = m(x[0], x[1], x[2], None, c["ii"], c["jj"], c["kk"], ix=c["ix"], jx=c["jx"],
                          gk=c["gk"], gij=c["gij"])
    assert none is None
    return x, (net, d, w)


@pytest.mark.parametrize("vonet", [False, True], ids=["Update", "VONet.update"])
def test_autograd_plumbing(ctx, vonet):
    case = (200, 882, "dpvo", 5)
    r = ctx.everything(case)
    c, cot = r["c"], [t.float() for t in r["cot"]]
    m = module(ctx, vonet=vonet)
    x, out = call(m, c)
    for o, want in zip(out, r["out"]):
        assert o.requires_grad and o.grad_fn is not None and torch.equal(o.detach()[0], want)
    sum((o[0] * t).sum() for o, t in zip(out, cot)).backward()
    got = [t.grad[0] for t in x] + [p.grad for p in m.parameters()]
    assert len(got) == 53
    for a, b in zip(got, r["got"]):
        assert torch.equal(a, b)
    # only what needs a gradient gets one
    m.zero_grad(set_to_none=True)
    for p in m.parameters():
        p.requires_grad_(False)
    x, out = call(m, c)
    (out[0][0] * cot[0]).sum().backward()
    assert all(p.grad is None for p in m.parameters()) and all(t.grad is not None for t in x)
    for p in m.parameters():
        p.requires_grad_(True)
    # no graph without the flag or under no_grad; the bits are the inference path's
    with torch.no_grad():
        _, quiet = call(m, c)
    _, plain = call(module(ctx, differentiable=False), c)
    e = ctx.ext
    host = e.pack_weights([t.cpu() for t in ctx.P((882, 1.0))[0]], 882, e.F32).to(ctx.dev)
    ws = torch.empty(e.workspace_bytes(200, 882), dtype=torch.uint8, device=ctx.dev)
    inf = [torch.full((200, n), float("nan"), device=ctx.dev) for n in (DIM, 2, 2)]
    e.plan(c["gk"], c["gij"], ws)
    e.forward(host, e.F32, c["net"], c["inp"], c["corr"], c["ix"], c["jx"], ws, *inf)
    for a, b, want in zip(quiet, plain, inf):
        assert a.grad_fn is None and not a.requires_grad and b.grad_fn is None
        assert torch.equal(a[0], want) and torch.equal(b[0], want)
    # one output used: the other cotangents arrive as None, which means zero
    x, out = call(m, c)
    (out[1][0] * cot[1]).sum().backward()
    z = ctx.backward((882, 1.0), c, r["saved"], [None, cot[1], None])
    for t, g in zip(x, z):
        assert torch.equal(t.grad[0], g)
    # an in-place optimiser-style step is seen by the next call
    before = [p.detach().clone() for p in m.parameters()]
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01 * torch.sign(p))
    _, out2 = call(m, c)
    P = {k: p.detach().double() for k, p in zip(ugr.names(882), m.parameters())}
    ref = update_ref.update_ref(P, c["net"].double(), c["inp"].double(), c["corr"].double(),
                                c["ix"], c["jx"], c["gk"], c["gij"])
    assert float((out2[0][0].detach().double() - ref[0]).abs().max()) <= 1e-5 * float(ref[0].abs().max())
    assert float((ref[0] - r["ref_out"][0]).abs().max()) > 1e-3 * float(ref[0].abs().max())
    assert any(not torch.equal(p.detach(), q) for p, q in zip(m.parameters(), before))


def test_differentiable_needs_fp32():
    from dpvo_amd.net import Update, VONet

    with pytest.raises(ValueError):
        Update(dtype=torch.float16, differentiable=True)
    with pytest.raises(ValueError):
        VONet(dtype=torch.float16, differentiable=True)
    assert not Update().differentiable


def test_no_host_synchronisation(ctx):
    r = ctx.everything((33, 882, "dpvo", 0))
    c, cot = r["c"], [t.float() for t in r["cot"]]
    m = module(ctx)

    def step():
        x, out = call(m, c)
        torch.autograd.backward(list(out), [t[None] for t in cot])
        return x

    step()  # warm-up: library load, kernel attributes
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    assert all(torch.isfinite(t.grad).all() for t in x)


@pytest.mark.parametrize("wname", ["F32", "F16"])
@pytest.mark.parametrize("K0", [49, 882])
def test_device_pack_equals_host_pack(ctx, K0, wname):
    x = ctx.ext
    wd = getattr(x, wname)
    host = [t.cpu().clone() for t in ctx.P((K0, 1.0))[0]]
    # zero, a subnormal half, a value under the smallest one, a tie, overflow
    host[38].view(-1)[:6] = torch.tensor([0.0, 1e-7, -3e-9, 2.0 ** -25, 65519.9, -1e6])
    host[46].view(-1)[:3] = torch.tensor([-0.0, 3e-6, 70000.0])
    want = x.pack_weights(host, K0, wd).to(ctx.dev)
    blob = torch.full((x.packed_bytes(K0, wd),), 0xAB, dtype=torch.uint8, device=ctx.dev)
    x.pack_weights_device([t.to(ctx.dev) for t in host], K0, wd, blob)
    assert torch.equal(blob, want)


def test_large_logits_stay_finite_and_within_the_bar(ctx):
    c = ctx.case(LOGIT_CASE)
    P1 = ctx.P((882, 1.0))[1]
    args = (c["net"].double(), c["inp"].double(), c["corr"].double(), c["ix"], c["jx"], c["gk"],
            c["gij"])
    base = update_ref.update_ref(P1, *args, return_logits=True)[3]
    key = (882, float(np.float32(80.0 / base)))
    logit = update_ref.update_ref(ctx.P(key)[1], *args, return_logits=True)[3]
    assert 60.0 < logit < 400.0, logit  # exp(80) overflows fp32 without the max subtraction
    r = ctx.everything(LOGIT_CASE, key)
    check_masks(r)
    check_grads(r["got"], r["ref"], r["g32"], 882, "large-logits")
