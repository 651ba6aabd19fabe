"""GPU: VONet.forward (the unroll of net.py:438-522), sequence_loss and
train_step, on 64 x 96 images (quarter resolution 16 x 24) with coords,
init_disps, edge_drop in {0, 1} and corr_dropout = 1 given, so that nothing is
random.  Weights: encoder_ref.formula_params and update_ref.formula_params.

The comparison (ii) is against the same unroll composed here from the parent's
public ops -- Patchifier, altcorr.corr, Update, ba.BA, pops.transform through
the lietorch ops and the torch / lietorch loss of train.py with a mask-free
mean.  Tolerance per compared quantity: S = the max-abs difference between two
runs of that composition that differ only in init_disps, multiplied by
(1 + 2^-20) in the second (a few ulps: what two correct fp32 orderings of
transform differ by; S also holds the run-to-run noise of the atomics of
A-CORR-BWD and of the patchify backward).  Bar: 8 S (two fused call sites per
step with gradient flow, a few ulps each, times a margin of 2), floor
2^-22 max|ref|.

The intrinsics of that comparison are (64, 64, 48, 32), the same for every
frame: (16, 16, 12, 8) at quarter resolution.  The reason is the yardstick.  At
step 0 the poses are the identity and the reprojected coordinates do not depend
on the depths at all, so the init_disps perturbation cannot stand for the
rounding of transform there; with a power-of-two focal length and an integer
principal point (x - cx) / fx fx + cx is exact in fp32, both orderings return
the patch coordinates to the bit at the identity, and the two unrolls part
where S starts to measure: at poses that have moved.  Measured on the MI355X
(6 frames x 4 patches, STEPS = 6, no edge drop), worst err / bound over the
loss, the 30 trajectory tensors and the 94 parameter gradients:
  intrinsics (64, 64, 48, 32)                       0.50 (loss)
  intrinsics (80 + f/4, 82 + f/4, 48 + f/4, 32 + f/4)  24.2 (update.gru.1.res.2.weight;
      trajectory 3.3, loss 3.0), where the parent's fp32 transform is an ulp off
      the patch coordinates at step 0 and S has nothing of it
  the latter against the parent composition with only its transform evaluated
      in fp64 by the same lietorch ops: trajectory and loss identical to the
      bit, gradients 0.010
so the whole difference is the rounding of the parent's fp32 transform.  The
second test keeps the general per-frame intrinsics in the unroll and compares
with that fp64-transform composition at the same bar.
"""
import functools

import pytest
import torch

import encoder_ref
import se3_restatement as L
import update_ref

pytestmark = pytest.mark.gpu

H, W = 64, 96
DIM = 384
N_PARAMS = 94  # every parameter tensor: 22 per encoder, 50 of the update operator


def make_net(dev, differentiable=True):
    from dpvo_amd.net import VONet

    net = VONet(dtype=torch.float32, differentiable=differentiable)
    Pf, Pi = encoder_ref.formula_params(128, "instance"), encoder_ref.formula_params(384, "none")
    net.patchify.fnet.load_state_dict({k: torch.as_tensor(v) for k, v in Pf.items()})
    net.patchify.inet.load_state_dict({k: torch.as_tensor(v) for k, v in Pi.items()})
    net.update.load_state_dict({k: torch.from_numpy(v)
                                for k, v in update_ref.formula_params(net.update.corr_dim).items()})
    return net.to(dev)


@functools.lru_cache(maxsize=None)
def inputs(N, ppi, intrinsics="general"):
    """CPU tensors: images in 0..255, ground-truth poses of a slow forward
    motion, disparities in 0.5..1.5, intrinsics that differ per frame
    ("general") or (64, 64, 48, 32) for every frame ("pow2")."""
    g = torch.Generator().manual_seed(100 * N + ppi)
    f = torch.arange(N, dtype=torch.float64)[:, None]
    xi = torch.cat([f * torch.tensor([0.03, -0.015, 0.01], dtype=torch.float64),
                    f * torch.tensor([0.004, -0.006, 0.003], dtype=torch.float64)], 1)
    return {
        "images": 255 * torch.rand(1, N, 3, H, W, generator=g),
        "poses": L.to_data(L.Exp(xi)).float()[None],
        "disps": 0.5 + torch.rand(1, N, H, W, generator=g),
        "intrinsics": ((torch.tensor([80.0, 82.0, 48.0, 32.0]) + 0.25 * f.float())[None]
                       if intrinsics == "general" else
                       torch.tensor([64.0, 64.0, 48.0, 32.0]).expand(1, N, 4).clone()),
        "coords": torch.stack([torch.randint(1, W // 4 - 1, (N, ppi), generator=g),
                               torch.randint(1, H // 4 - 1, (N, ppi), generator=g)], -1).float(),
        "init_disps": 0.5 + torch.rand(1, N * ppi, generator=g),
    }


def forward(net, x, dev, **kw):
    from dpvo_amd.lietorch import SE3

    kw.setdefault("init_disps", x["init_disps"].to(dev))
    kw.setdefault("edge_drop", 0)
    return net(x["images"].to(dev), SE3(x["poses"].to(dev)), x["disps"].to(dev),
               x["intrinsics"].to(dev), coords=x["coords"].to(dev), corr_dropout=1, **kw)


def flat(traj):
    """name -> tensor for every tensor of a trajectory."""
    out = {}
    for i, (v, c, cg, G, P, kl) in enumerate(traj):
        out.update({f"step{i}.valid": v, f"step{i}.coords": c, f"step{i}.coords_gt": cg,
                    f"step{i}.Gs": G.data, f"step{i}.Ps": P.data})
    return {k: t.detach() for k, t in out.items()}


def grads(net):
    return {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def clear(net):
    for p in net.parameters():
        p.grad = None


# ------------------------------------------------- the parent's composition

def flatmeshgrid(a, b):
    x, y = torch.meshgrid(a, b, indexing="ij")
    return x.reshape(-1), y.reshape(-1)


def parent_forward(net, x, dev, STEPS, init_frames, drop, init_disps, structure_only=False):
    """net.py:438-522 on the parent's ops; ``drop`` replaces the 10 % draw."""
    from dpvo_amd import altcorr, projective_ops as pops
    from dpvo_amd.ba import BA
    from dpvo_amd.lietorch import SE3

    images = 2 * (x["images"].to(dev) / 255.0) - 0.5
    intrinsics = x["intrinsics"].to(dev) / 4.0
    disps = x["disps"].to(dev)[:, :, 1::4, 1::4].float()
    poses = SE3(x["poses"].to(dev))
    fmap, gmap, imap, patches, ix = net.patchify(images, disps=disps, coords=x["coords"].to(dev))
    b, N, c, h, w = fmap.shape
    p = net.P
    pyramid = [torch.nn.functional.avg_pool2d(fmap.view(b * N, c, h, w), l, stride=l)
               .view(b, N, c, h // l, w // l) for l in (1, 4)]

    def corr_fn(ii, jj, coords):
        cs = [altcorr.corr(gmap, pyramid[i], coords / l, ii, jj, 3, 1) for i, l in enumerate((1, 4))]
        return torch.stack(cs, -1).view(1, len(ii), -1)

    patches_gt = patches.clone()
    Ps = poses
    patches = patches.clone()
    patches[..., 2, :, :] = init_disps.to(dev).view(1, -1)[..., None, None]
    kk, jj = flatmeshgrid(torch.where(ix < init_frames)[0], torch.arange(0, init_frames, device=dev))
    ii = ix[kk]
    imap = imap.view(b, -1, DIM)
    net_h = torch.zeros(b, len(kk), DIM, device=dev)
    Gs = SE3.IdentityLike(poses)
    if structure_only:
        Gs.data[:] = poses.data[:]
    traj = []
    bounds = [-64, -64, w + 64, h + 64]
    while len(traj) < STEPS:
        Gs = Gs.detach()
        patches = patches.detach()
        n = int(ii.max()) + 1
        if len(traj) >= init_frames and n < N:
            if not structure_only:
                Gs = SE3(Gs.data.clone())
                Gs.data[:, n] = Gs.data[:, n - 1]
            kk1, jj1 = flatmeshgrid(torch.where(ix < n)[0], torch.arange(n, n + 1, device=dev))
            kk2, jj2 = flatmeshgrid(torch.where(ix == n)[0], torch.arange(0, n + 1, device=dev))
            ii = torch.cat([ix[kk1], ix[kk2], ii])
            jj = torch.cat([jj1, jj2, jj])
            kk = torch.cat([kk1, kk2, kk])
            net_h = torch.cat([torch.zeros(b, len(kk1) + len(kk2), DIM, device=dev), net_h], dim=1)
            if drop:
                k = (ii != (n - 4)) & (jj != (n - 4))
                ii, jj, kk, net_h = ii[k], jj[k], kk[k], net_h[:, k]
            patches = patches.clone()
            patches[:, ix == n, 2] = torch.median(patches[:, (ix == n - 1) | (ix == n - 2), 2])
            n = int(ii.max()) + 1
        coords = pops.transform(Gs, patches, intrinsics, ii, jj, kk)
        coords1 = coords.permute(0, 1, 4, 2, 3).contiguous()
        corr = corr_fn(kk, jj, coords1)
        net_h, (delta, weight, _) = net.update(net_h, imap[:, kk], corr, None, ii, jj, kk)
        target = coords[..., p // 2, p // 2, :] + delta
        for _ in range(2):
            Gs, patches = BA(Gs, patches, intrinsics, target, weight, 1e-4, ii, jj, kk, bounds,
                             ep=10, fixedp=1, structure_only=structure_only)
        dij = (ii - jj).abs()
        k = (dij > 0) & (dij <= 2)
        coords = pops.transform(Gs, patches, intrinsics, ii[k], jj[k], kk[k])
        coords_gt, valid, _ = pops.transform(Ps, patches_gt, intrinsics, ii[k], jj[k], kk[k],
                                             jacobian=True)
        traj.append((valid, coords, coords_gt, Gs[:, :n], Ps[:, :n], torch.zeros((), device=dev)))
    return traj


def kabsch_umeyama(A, B):  # train.py:31-41
    n, m = A.shape
    EA, EB = torch.mean(A, axis=0), torch.mean(B, axis=0)
    VarA = torch.mean((A - EA).norm(dim=1) ** 2)
    Hm = ((A - EA).T @ (B - EB)) / n
    U, D, VT = torch.svd(Hm)
    return VarA / torch.trace(torch.diag(D))


def parent_loss(traj, P=3, structure_only=False):
    """train.py:85-118; the masked mean as sum(e m) / sum(m)."""
    loss = 0.0
    for i, (v, x, y, P1, P2, kl) in enumerate(traj):
        e = (x - y).norm(dim=-1).reshape(-1, P * P).min(dim=-1).values
        m = (v > 0.5).reshape(-1).to(e.dtype)
        N = P1.shape[1]
        ii, jj = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
        ii, jj = ii.reshape(-1).to(e.device), jj.reshape(-1).to(e.device)
        k = ii != jj
        ii, jj = ii[k], jj[k]
        P1, P2 = P1.inv(), P2.inv()
        t1, t2 = P1.matrix()[..., :3, 3], P2.matrix()[..., :3, 3]
        s = kabsch_umeyama(t2[0], t1[0]).detach().clamp(max=10.0)
        P1 = P1.scale(s.view(1, 1))
        dP = P1[:, ii].inv() * P1[:, jj]
        dG = P2[:, ii].inv() * P2[:, jj]
        e1 = (dP * dG.inv()).log()
        tr, ro = e1[..., 0:3].norm(dim=-1), e1[..., 3:6].norm(dim=-1)
        loss = loss + 0.1 * (e * m).sum() / m.sum()
        if not structure_only and i >= 2:
            loss = loss + 10.0 * (tr.mean() + ro.mean())
    return loss


# ------------------------------------------------------------------ (i)

def schedule_shapes(N, ppi, steps, init_frames, drop):
    from dpvo_amd.net import training_schedule

    out = []
    for ii, jj, kk, n in training_schedule(N, ppi, steps, init_frames, drop=lambda s: drop):
        d = (ii - jj).abs()
        out.append((int(((d > 0) & (d <= 2)).sum()), n))
    return out


@pytest.mark.parametrize("edge_drop", [0, 1])
def test_structure(gpu, edge_drop):
    net, x = make_net(gpu), inputs(10, 4)
    with torch.no_grad():
        traj = forward(net, x, gpu, STEPS=10, edge_drop=edge_drop)
    assert len(traj) == 10
    want = schedule_shapes(10, 4, 10, 8, bool(edge_drop))
    assert [w[0] for w in want] == [104] * 8 + ([88, 80] if edge_drop else [120, 136])
    eye = torch.tensor([0.0, 0, 0, 0, 0, 0, 1], device=gpu)
    for (v, c, cg, G, P, kl), (E, n) in zip(traj, want):
        assert v.shape == (1, E) and c.shape == (1, E, 3, 3, 2) and cg.shape == (1, E, 3, 3, 2)
        assert G.data.shape == (1, n, 7) and P.data.shape == (1, n, 7)
        assert kl.dim() == 0 and float(kl) == 0
        for t in (v, c, cg, G.data, P.data):
            assert t.isfinite().all()
        assert torch.equal(G.data[0, 0], eye)
        assert torch.equal(P.data, x["poses"].to(gpu)[:, :n])


def test_structure_only_keeps_the_poses(gpu):
    net, x = make_net(gpu), inputs(10, 4)
    with torch.no_grad():
        traj = forward(net, x, gpu, STEPS=10, structure_only=True)
    for (v, c, cg, G, P, kl), (E, n) in zip(traj, schedule_shapes(10, 4, 10, 8, False)):
        assert torch.equal(G.data, x["poses"].to(gpu)[:, :n])
        assert c.isfinite().all() and c.shape == (1, E, 3, 3, 2)


def test_batch_size_one_only(gpu):
    net, x = make_net(gpu), inputs(6, 4)
    from dpvo_amd.lietorch import SE3

    with pytest.raises(ValueError):
        net(x["images"].to(gpu).repeat(2, 1, 1, 1, 1), SE3(x["poses"].to(gpu)), x["disps"].to(gpu),
            x["intrinsics"].to(gpu), STEPS=1, init_frames=4, coords=x["coords"].to(gpu))


# ------------------------------------------------------------------ (ii)

def fused_run(net, x, dev, drop):
    from dpvo_amd.training import sequence_loss

    clear(net)
    traj = forward(net, x, dev, STEPS=6, init_frames=4, edge_drop=int(drop))
    loss, _ = sequence_loss(traj)
    loss.backward()
    return loss.detach(), flat(traj), grads(net)


def parent_run(net, x, dev, drop, init_disps):
    clear(net)
    traj = parent_forward(net, x, dev, 6, 4, drop, init_disps)
    loss = parent_loss(traj)
    loss.backward()
    return loss.detach(), flat(traj), grads(net)


class transform_in_fp64:
    """Inside: pops.transform evaluates in fp64 (the same lietorch ops on
    doubles) and rounds its outputs to fp32 once."""

    def __enter__(self):
        from dpvo_amd import projective_ops as pops
        from dpvo_amd.lietorch import SE3

        self.pops, self.orig = pops, pops.transform

        def transform(poses, patches, intr, ii, jj, kk, **kw):
            out = self.orig(SE3(poses.data.double()), patches.double(), intr.double(), ii, jj, kk,
                            **kw)
            if isinstance(out, tuple):
                return (out[0].float(), out[1].float()) + ((None,) if len(out) > 2 else ())
            return out.float()

        pops.transform = transform

    def __exit__(self, *exc):
        self.pops.transform = self.orig


def compare(new, ref, per, tag, check=True):
    worst, bad = (-1.0, ""), {}
    for fam, a, b, c in (("loss", {"loss": new[0]}, {"loss": ref[0]}, {"loss": per[0]}),
                         ("traj", new[1], ref[1], per[1]), ("grad", new[2], ref[2], per[2])):
        assert a.keys() == b.keys()
        for name in b:
            S = float((c[name] - b[name]).abs().max())
            scale = float(b[name].abs().max())
            err = float((a[name] - b[name]).abs().max())
            bound = max(8 * S, 2.0 ** -22 * scale)
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
            print(f"PARITY vonet {tag} {fam} {name}: err {err:.3e} S {S:.3e} "
                  f"max|ref| {scale:.3e} err/bound {ratio:.3f}")
            worst = max(worst, (ratio, name))
            if not err <= bound:
                bad[name] = (err, bound)
    print(f"PARITY vonet {tag} worst err/bound {worst[0]:.3f} at {worst[1]}")
    if check:
        assert not bad, bad
    return worst


@pytest.mark.parametrize("drop", [False, True])
def test_matches_the_parent_composition(gpu, drop):
    net, x = make_net(gpu), inputs(6, 4, "pow2")
    new = fused_run(net, x, gpu, drop)
    ref = parent_run(net, x, gpu, drop, x["init_disps"])
    per = parent_run(net, x, gpu, drop, x["init_disps"] * (1 + 2.0 ** -20))
    assert len(ref[2]) == N_PARAMS and len(ref[1]) == 30
    compare(new, ref, per, f"drop={int(drop)}")


def test_matches_the_composition_with_an_fp64_transform(gpu):
    """Per-frame intrinsics; S from the parent's fp32 composition as above."""
    net, x = make_net(gpu), inputs(6, 4, "general")
    new = fused_run(net, x, gpu, False)
    ref32 = parent_run(net, x, gpu, False, x["init_disps"])
    per32 = parent_run(net, x, gpu, False, x["init_disps"] * (1 + 2.0 ** -20))
    with transform_in_fp64():
        ref = parent_run(net, x, gpu, False, x["init_disps"])
    # the bar's S: between the two fp32 runs, applied around the fp64-transform run
    per = tuple({k: ref[i][k] + (per32[i][k] - ref32[i][k]) for k in ref[i]} if i else
                ref[0] + (per32[0] - ref32[0]) for i in range(3))
    compare(new, ref, per, "fp64-transform")
    # printed, not asserted: the issue's fp32 comparison at these general
    # intrinsics, where S holds nothing of step 0's transform rounding
    # (measured: 24.2, see the module docstring)
    compare(new, ref32, per32, "general-intrinsics-fp32 (not asserted)", check=False)


# ------------------------------------------------------------------ (iii)

def structural_zeros(net):
    """The zeros the update and encoder tests name: the biases of the
    instance-norm encoder's convs 0..9 (exact) and agg_*.g.bias (rounding noise)."""
    fnet = [n for n, _ in net.patchify.fnet.named_parameters()]
    return {"patchify.fnet." + n for i, n in enumerate(fnet) if i < 20 and n.endswith("bias")} | \
        {"update.agg_kk.g.bias", "update.agg_ij.g.bias"}


def test_all_parameters_receive_a_gradient(gpu):
    net, x = make_net(gpu), inputs(6, 4)
    loss, traj, g = fused_run(net, x, gpu, False)
    assert len(g) == N_PARAMS and loss.isfinite()
    zeros = structural_zeros(net)
    assert len(zeros) == 12 and zeros <= set(g)
    for name, t in g.items():
        assert t.isfinite().all(), name
        if name not in zeros:
            assert t.abs().max() > 0, name


def test_detach_points_and_inference_mode(gpu):
    from dpvo_amd.lietorch import SE3
    from dpvo_amd.training import sequence_loss

    net, x = make_net(gpu), inputs(6, 4)
    loss, traj, g = fused_run(net, x, gpu, False)
    # ground-truth poses that require grad change nothing: Gs / patches are detached per step
    clear(net)
    Pd = x["poses"].to(gpu).requires_grad_()
    t2 = net(x["images"].to(gpu), SE3(Pd), x["disps"].to(gpu), x["intrinsics"].to(gpu), STEPS=6,
             init_frames=4, coords=x["coords"].to(gpu), init_disps=x["init_disps"].to(gpu),
             edge_drop=0, corr_dropout=1)
    for k, v in flat(t2).items():
        assert torch.equal(v, traj[k]), k
    # two forward calls are bit-identical; so is differentiable=False, without a graph
    plain = make_net(gpu, differentiable=False)
    t3 = forward(plain, x, gpu, STEPS=6, init_frames=4)
    for v, c, cg, G, P, kl in t3:
        assert c.grad_fn is None and G.data.grad_fn is None and not c.requires_grad
    for k, v in flat(t3).items():
        assert torch.equal(v, traj[k]), k
    with torch.no_grad():
        t4 = forward(net, x, gpu, STEPS=6, init_frames=4)
    for k, v in flat(t4).items():
        assert torch.equal(v, traj[k]), k
    assert sequence_loss(t2)[0].isfinite()
    # structure only: Gs starts as a detached copy of the poses
    with torch.no_grad():
        so = forward(net, x, gpu, STEPS=6, init_frames=4, structure_only=True)
    so2 = net(x["images"].to(gpu), SE3(Pd), x["disps"].to(gpu), x["intrinsics"].to(gpu), STEPS=6,
              init_frames=4, coords=x["coords"].to(gpu), init_disps=x["init_disps"].to(gpu),
              edge_drop=0, corr_dropout=1, structure_only=True)
    for k, v in flat(so2).items():
        assert torch.equal(v, flat(so)[k]), k


# ------------------------------------------------------------------ (iv)

def test_train_step(gpu):
    from dpvo_amd.lietorch import SE3
    from dpvo_amd.training import train_step

    net, x = make_net(gpu), inputs(6, 4)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    args = (x["images"].to(gpu), SE3(x["poses"].to(gpu)), x["disps"].to(gpu),
            x["intrinsics"].to(gpu))
    kw = dict(steps=6, init_frames=4, coords=x["coords"].to(gpu),
              init_disps=x["init_disps"].to(gpu), edge_drop=0, corr_dropout=1)
    loss, metrics = train_step(net, opt, *args, **kw)
    assert loss.isfinite() and loss.device.type == "cuda"
    assert set(metrics) == {"loss", "kl", "px1", "ro", "tr", "r1", "r2", "t1", "t2"}
    assert all(isinstance(v, torch.Tensor) and v.device.type == "cuda" for v in metrics.values())
    changed = [n for n, p in net.named_parameters() if not torch.equal(p, before[n])]
    # only the structural zeros may stay as they were
    assert set(before) - set(changed) <= structural_zeros(net), set(before) - set(changed)
    loss2, _ = train_step(net, opt, *args, **kw)
    assert loss2.isfinite()


# ------------------------------------------------------------------ (v)

def test_no_host_synchronisation(gpu):
    from dpvo_amd.lietorch import SE3
    from dpvo_amd.training import sequence_loss

    net, x = make_net(gpu), inputs(6, 4)
    fused_run(net, x, gpu, False)  # warm-up
    clear(net)
    args = (x["images"].to(gpu), SE3(x["poses"].to(gpu)), x["disps"].to(gpu),
            x["intrinsics"].to(gpu))
    kw = dict(STEPS=6, init_frames=4, coords=x["coords"].to(gpu),
              init_disps=x["init_disps"].to(gpu), edge_drop=0, corr_dropout=1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        traj = net(*args, **kw)
        loss, metrics = sequence_loss(traj)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loss.isfinite()
