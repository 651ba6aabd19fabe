"""GPU: the flow loss and the pose loss of dpvo_amd.training (train.hip)
against the fp64 restatements of train_ref: values and gradients within
1e-5 max|ref| per tensor, the bar the encoder and BA-layer gradient tests use
for fp64-inside kernels; repeats bit-identical; no host synchronisation."""
import functools
import math

import pytest
import torch

import se3_restatement as L
import train_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-5
GAP = 1e-3  # the two smallest errors of every valid edge differ by this much in fp64


def close(got, ref, name):
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    print(f"PARITY train_loss {name}: err {err:.3e} max|ref| {scale:.3e} bar {BAR * scale:.3e}")
    assert err <= BAR * scale, (name, err, scale)


# ------------------------------------------------------------------ flow loss

@functools.lru_cache(maxsize=None)
def flow_case(E, P, kind):
    """kind 'mix': valid and invalid edges, edge 0 valid with one exactly-zero
    difference; 'none': every edge invalid."""
    g = torch.Generator().manual_seed(7 * E + P)
    PP = P * P
    y = 100 * torch.rand(E, PP, 2, generator=g, dtype=torch.float64)
    rank = torch.stack([torch.randperm(PP, generator=g) for _ in range(E)]).double()
    mag = 0.1 + 0.07 * rank + 0.02 * torch.rand(E, PP, generator=g, dtype=torch.float64)
    ang = 2 * math.pi * torch.rand(E, PP, generator=g, dtype=torch.float64)
    x = y + mag[..., None] * torch.stack([ang.cos(), ang.sin()], -1)
    x, y = x.float(), y.float()
    x[0, PP - 1] = y[0, PP - 1]  # an exactly-zero difference: the minimum of edge 0
    valid = (torch.rand(E, generator=g) < 0.6).float()
    valid[0] = 1.0
    if kind == "none":
        valid[:] = 0.0
    return x.view(E, P, P, 2), y.view(E, P, P, 2), valid


def flow_run(x, y, valid, dev, g=2.5):
    from dpvo_amd.training import flow_loss

    xd = x.to(dev)[None].requires_grad_()
    loss, count, emin = flow_loss(xd, y.to(dev)[None], valid.to(dev)[None])
    (gx,) = torch.autograd.grad(loss * g, xd)
    return loss, count, emin, gx[0]


@pytest.mark.parametrize("kind", ["mix", "none"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("E", [1, 64, 130])
def test_flow_loss(gpu, E, P, kind):
    x, y, valid = flow_case(E, P, kind)
    ref = R.flow_loss(x, y, valid, g=2.5)
    if P > 1:  # the argmin is not a rounding question
        two = ref["errors"].sort(dim=1).values[:, :2]
        assert ((two[:, 1] - two[:, 0])[valid > 0.5] >= GAP).all()
    assert ref["errors"][0].min() == 0
    loss, count, emin, gx = flow_run(x, y, valid, gpu)
    assert loss.dim() == 0 and count.dim() == 0 and emin.shape == (E,)
    assert int(count) == ref["count"]
    if kind == "none":  # the deviation from the reference: 0, not NaN
        assert float(loss.detach()) == 0.0 and (gx == 0).all() and ref["loss"] == 0
    close(loss, ref["loss"], f"flow E{E} P{P} {kind} loss")
    close(emin, ref["emin"], f"flow E{E} P{P} {kind} emin")
    close(gx, ref["g_coords"], f"flow E{E} P{P} {kind} g_coords")
    assert (gx[0] == 0).all()  # edge 0: the minimum is the exactly-zero difference
    assert (gx[valid < 0.5] == 0).all()
    assert int((gx.flatten(1).abs().sum(1) > 0).sum()) == max(ref["count"] - 1, 0)


def test_flow_loss_ties_take_the_lowest_point(gpu):
    y = torch.zeros(2, 3, 3, 2)
    x = torch.zeros(2, 3, 3, 2)
    x[..., 0] = 3.0
    x[0, 1, 1, 0] = x[0, 2, 0, 0] = 1.0  # points 4 and 6 tie
    loss, count, emin, gx = flow_run(x, y, torch.ones(2), gpu, g=1.0)
    assert float(loss) == 2.0 and emin.tolist() == [1.0, 3.0]
    assert gx[0].reshape(9, 2)[4].tolist() == [0.5, 0.0] and gx[0].abs().sum() == 0.5
    assert gx[1].reshape(9, 2)[0].tolist() == [0.5, 0.0] and gx[1].abs().sum() == 0.5


def test_flow_loss_takes_the_centre_of_a_full_valid_map(gpu):
    from dpvo_amd.training import flow_loss

    x, y, valid = flow_case(64, 3, "mix")
    full = torch.zeros(64, 3, 3)
    full[:, 1, 1] = valid
    a = flow_loss(x.to(gpu)[None], y.to(gpu)[None], valid.to(gpu)[None])
    b = flow_loss(x.to(gpu)[None], y.to(gpu)[None], full.to(gpu)[None])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ pose loss

@functools.lru_cache(maxsize=None)
def pose_case(n, kind):
    """Ground truth: distinct translations, rotations up to about 1 rad.  The
    estimate: the ground truth with its translations halved, moved by a
    tangent step with rotation up to about 1 rad.  'twin': poses 0 and 1 are
    bitwise identical in both sets (e_01 = e_10 = 0); 'clamp': estimated
    translations 100 times smaller, so s = 10."""
    g = torch.Generator().manual_seed(31 * n + len(kind))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    xi = torch.cat([2.0 * rnd(n, 3), 0.5 * rnd(n, 3).clamp(-1, 1)], 1)
    Ps = L.to_data(L.Exp(xi))
    step = torch.cat([0.1 * rnd(n, 3), 0.45 * rnd(n, 3).clamp(-1.2, 1.2)], 1)
    Gm = L.Exp(step) @ L.Exp(xi)
    G = L.to_data(Gm)
    Gi = L.inv(L.from_data(G))  # scale the translation of the inverse, as the loss reads it
    Gi[:, :3, 3] *= 0.01 if kind == "clamp" else 0.5
    G = L.to_data(L.inv(Gi))
    G, Ps = G.float(), Ps.float()
    if kind == "twin":
        G[1], Ps[1] = G[0], Ps[0]
    return G, Ps


def pose_run(G, Ps, dev, g_tr=1.0, g_ro=1.0):
    from dpvo_amd.lietorch import SE3
    from dpvo_amd.training import pose_loss

    Gd = G.to(dev)[None].requires_grad_()
    tr, ro, trp, rop, s = pose_loss(SE3(Gd), SE3(Ps.to(dev)[None]))
    (gG,) = torch.autograd.grad(g_tr * tr + g_ro * ro, Gd)
    return tr, ro, trp, rop, s, gG[0]


# two bitwise identical poses at n = 2 leave no variance: s = 0 / 0 is NaN in the
# reference's arithmetic and in the kernel's, so the twin case starts at n = 3
POSE_CASES = [(n, kind) for n in (2, 3, 9, 32) for kind in ("distinct", "twin", "clamp")
              if (n, kind) != (2, "twin")]


@pytest.mark.parametrize("n,kind", POSE_CASES)
def test_pose_loss(gpu, n, kind):
    G, Ps = pose_case(n, kind)
    ref = R.pose_loss(G, Ps, g_tr=0.7, g_ro=1.3)
    t_gt = L.inv(L.from_data(Ps))[:, :3, 3]
    if kind != "twin":
        assert torch.cdist(t_gt, t_gt)[~torch.eye(n, dtype=torch.bool)].min() > 1e-2
    if kind == "clamp":
        assert float(ref["s"]) == 10.0
    else:
        assert float(ref["s"]) < 10.0
    tr, ro, trp, rop, s, gG = pose_run(G, Ps, gpu, 0.7, 1.3)
    assert trp.shape == (n * (n - 1),) and rop.shape == (n * (n - 1),)
    tag = f"pose n{n} {kind}"
    close(s, ref["s"], tag + " s")
    close(tr, ref["tr"], tag + " tr")
    close(ro, ref["ro"], tag + " ro")
    close(trp, ref["tr_pairs"], tag + " tr_pairs")
    close(rop, ref["ro_pairs"], tag + " ro_pairs")
    assert gG.isfinite().all() and (gG[:, 6] == 0).all()
    close(gG[:, :6], ref["g_G"], tag + " g_G")
    if kind == "twin":  # e_01 = e_10 = 0 exactly; its gradient is zero, not NaN
        assert trp[0] == 0 and rop[0] == 0 and trp[n - 1] == 0 and rop[n - 1] == 0


def test_pose_loss_limits(gpu):
    from dpvo_amd.training import pose_loss

    G, Ps = pose_case(2, "distinct")
    Gd = G[:1].to(gpu)[None].requires_grad_()
    tr, ro, trp, rop, s = pose_loss(Gd, Ps[:1].to(gpu)[None])  # n = 1: zeros, nothing launched
    assert float(tr) == 0 and float(ro) == 0 and trp.numel() == 0
    (gG,) = torch.autograd.grad(tr + ro, Gd)
    assert (gG == 0).all()
    big = torch.zeros(1, 33, 7, device=gpu)
    big[..., 6] = 1
    with pytest.raises(RuntimeError):
        pose_loss(big, big)


def test_repeats_are_bit_identical(gpu):
    x, y, valid = flow_case(130, 3, "mix")
    a, b = flow_run(x, y, valid, gpu), flow_run(x, y, valid, gpu)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    G, Ps = pose_case(32, "distinct")
    a, b = pose_run(G, Ps, gpu), pose_run(G, Ps, gpu)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_no_host_synchronisation(gpu):
    from dpvo_amd.training import flow_loss, pose_loss

    x, y, valid = flow_case(130, 3, "mix")
    G, Ps = pose_case(9, "distinct")
    flow_run(x, y, valid, gpu)  # warm-up
    pose_run(G, Ps, gpu)
    xd, yd, vd = x.to(gpu)[None].requires_grad_(), y.to(gpu)[None], valid.to(gpu)[None]
    Gd, Pd = G.to(gpu)[None].requires_grad_(), Ps.to(gpu)[None]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, count, emin = flow_loss(xd, yd, vd)
        tr, ro, trp, rop, s = pose_loss(Gd, Pd)
        gx, gG = torch.autograd.grad(loss + tr + ro, (xd, Gd))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert gx.isfinite().all() and gG.isfinite().all()
