"""Timing of the training step's fused pieces and of one whole train_step at
the reference's training shape: 15 frames of 480 x 640, 80 patches per image,
STEPS = 18.  Synthetic images, formula weights (tests/encoder_ref.py,
tests/update_ref.py).  GPU only.

  1. projective_ops.transform_fused against projective_ops.transform through
     the lietorch ops: E = 4320, P = 3 forward + backward (the loss edges of
     the last step), E = 18000, P = 3 forward only (all edges of the last step)
  2. training.flow_loss / pose_loss against the torch / lietorch formulation
     of train.py:85-113 (E = 4320, n = 15), forward + backward
  3. one train_step: wall time, and the device time of its kernels split by
     component (encoders, corr, update, BA, transform, losses, the rest),
     forward and backward, from torch.profiler

HIP events, warm-up, medians of alternating repetitions.

    python scripts/train_step_bench.py [--reps 30] [--frames 15] [--height 480] [--width 640]
"""
import argparse
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402

import dpvo_amd  # noqa: E402,F401
import encoder_ref  # noqa: E402
import update_ref  # noqa: E402
from dpvo_amd import projective_ops as pops  # noqa: E402
from dpvo_amd import training  # noqa: E402
from dpvo_amd.lietorch import SE3  # noqa: E402
from dpvo_amd.net import VONet, training_schedule  # noqa: E402


def timed_pair(fa, fb, reps):
    """Medians (us) of fa and fb, alternating, after a warm-up."""
    for _ in range(5):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
    ta.sort()
    tb.sort()
    return round(ta[len(ta) // 2], 1), round(tb[len(tb) // 2], 1)


def scene(N, ppi, h, w, dev, seed=0):
    """Poses of a slow forward motion, patches on a quarter-resolution grid."""
    g = torch.Generator().manual_seed(seed)
    f = torch.arange(N, dtype=torch.float32)[:, None]
    xi = torch.cat([f * torch.tensor([0.03, -0.015, 0.01]), f * torch.tensor([0.004, -0.006, 0.003])], 1)
    poses = SE3.exp(xi.to(dev)[None]).data
    M = N * ppi
    x = torch.randint(1, w - 1, (M,), generator=g).float()
    y = torch.randint(1, h - 1, (M,), generator=g).float()
    d = 0.5 + torch.rand(M, generator=g)
    off = torch.arange(3).float() - 1
    patches = torch.stack([x[:, None, None] + off[None, None, :].expand(M, 3, 3),
                           y[:, None, None] + off[None, :, None].expand(M, 3, 3),
                           d[:, None, None].expand(M, 3, 3)], 1)
    intr = torch.tensor([w / 2.0, w / 2.0, w / 2.0, h / 2.0]).expand(1, N, 4)
    return poses, patches.to(dev)[None].contiguous(), intr.to(dev).contiguous()


def bench_transform(args, dev):
    N, ppi = args.frames, 80
    ii, jj, kk, _ = training_schedule(N, ppi, 18, drop=lambda s: False)[-1]
    d = (ii - jj).abs()
    k = (d > 0) & (d <= 2)
    poses, patches, intr = scene(N, ppi, args.height // 4, args.width // 4, dev)
    for name, idx, backward in (("loss edges", k, True), ("all edges", torch.ones_like(k), False)):
        i, j, q = ii[idx].to(dev), jj[idx].to(dev), kk[idx].to(dev)
        cot = torch.randn(len(i), 3, 3, 2, device=dev)[None]

        def run(fn):
            def f():
                P, K = poses.clone().requires_grad_(backward), patches.clone().requires_grad_(backward)
                with torch.set_grad_enabled(backward):
                    c = fn(SE3(P), K, intr, i, j, q)
                    if backward:
                        (c * cot).sum().backward()
                return c.detach(), P.grad, K.grad
            return f

        fused, comp = run(pops.transform_fused), run(pops.transform)
        a, b = fused(), comp()
        tf, tc = timed_pair(fused, comp, args.reps)
        out = {"bench": "transform", "edges": name, "E": len(i), "P": 3, "backward": backward,
               "fused_us": tf, "composed_us": tc,
               "coords_max_abs_diff": float((a[0] - b[0]).abs().max())}
        if backward:
            out["g_poses_rel_diff"] = float((a[1] - b[1]).abs().max() / b[1].abs().max())
            out["g_patches_rel_diff"] = float((a[2] - b[2]).abs().max() / b[2].abs().max())
        print(json.dumps(out), flush=True)


def kabsch_umeyama(A, B):  # train.py:31-41
    n = A.shape[0]
    EA, EB = A.mean(0), B.mean(0)
    VarA = ((A - EA).norm(dim=1) ** 2).mean()
    H = ((A - EA).T @ (B - EB)) / n
    return VarA / torch.trace(torch.diag(torch.svd(H)[1]))


def torch_flow_loss(x, y, v):  # train.py:87-88, 115
    e = (x - y).norm(dim=-1)
    return e.reshape(-1, 9)[(v > 0.5).reshape(-1)].min(dim=-1).values.mean()


def torch_pose_loss(P1, P2, ii, jj):  # train.py:99-113, 117
    P1, P2 = P1.inv(), P2.inv()
    t1, t2 = P1.matrix()[..., :3, 3], P2.matrix()[..., :3, 3]
    s = kabsch_umeyama(t2[0], t1[0]).detach().clamp(max=10.0)
    P1 = P1.scale(s.view(1, 1))
    e1 = ((P1[:, ii].inv() * P1[:, jj]) * (P2[:, ii].inv() * P2[:, jj]).inv()).log()
    return e1[..., 0:3].norm(dim=-1).mean() + e1[..., 3:6].norm(dim=-1).mean()


def bench_losses(args, dev):
    N, E = args.frames, 4320
    g = torch.Generator().manual_seed(2)
    y = 100 * torch.rand(1, E, 3, 3, 2, generator=g)
    x0 = (y + torch.randn(1, E, 3, 3, 2, generator=g)).to(dev)
    y, v = y.to(dev), (torch.rand(1, E, generator=g) < 0.9).float().to(dev)

    def flow(fn):
        def f():
            x = x0.clone().requires_grad_()
            out = fn(x, y, v)
            out = out[0] if isinstance(out, tuple) else out
            out.backward()
            return out.detach(), x.grad
        return f

    fused, comp = flow(training.flow_loss), flow(torch_flow_loss)
    a, b = fused(), comp()
    tf, tc = timed_pair(fused, comp, args.reps)
    print(json.dumps({"bench": "flow_loss", "E": E, "P": 3, "fused_us": tf, "composed_us": tc,
                      "loss_diff": float((a[0] - b[0]).abs()),
                      "grad_max_abs_diff": float((a[1] - b[1]).abs().max())}), flush=True)

    Ps, _, _ = scene(N, 1, 8, 8, dev)
    G0 = SE3.exp(0.05 * torch.randn(1, N, 6, generator=g).to(dev)).mul(SE3(Ps)).data
    ii, jj = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    ii, jj = ii[ii != jj].to(dev), jj[ii != jj].to(dev)

    def pose(which):
        def f():
            G = G0.clone().requires_grad_()
            if which == "fused":
                tr, ro = training.pose_loss(SE3(G), SE3(Ps))[:2]
                out = tr + ro
            else:
                out = torch_pose_loss(SE3(G), SE3(Ps), ii, jj)
            out.backward()
            return out.detach(), G.grad
        return f

    fused, comp = pose("fused"), pose("torch")
    a, b = fused(), comp()
    tf, tc = timed_pair(fused, comp, args.reps)
    print(json.dumps({"bench": "pose_loss", "n": N, "fused_us": tf, "composed_us": tc,
                      "loss_rel_diff": float((a[0] - b[0]).abs() / b[0].abs()),
                      "grad_rel_diff": float((a[1] - b[1]).abs().max() / b[1].abs().max())}),
          flush=True)


FWD = {"encoders": "fwd:encoders", "corr": "fwd:corr", "update": "fwd:update", "BA": "fwd:BA",
       "transform": "fwd:transform", "losses": "fwd:losses"}
BWD = {"_EncoderFunctionBackward": "encoders", "PatchLayerBackward": "encoders",
       "CorrLayerBackward": "corr", "_UpdateFunctionBackward": "update", "_BALayerBackward": "BA",
       "_TransformFusedBackward": "transform", "_FlowLossBackward": "losses",
       "_PoseLossBackward": "losses"}


def labelled(obj, name, label):
    fn = getattr(obj, name)

    def wrapper(*a, **kw):
        with torch.profiler.record_function(label):
            return fn(*a, **kw)

    setattr(obj, name, wrapper)
    return lambda: setattr(obj, name, fn)


def device_us(e):
    return float(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total)


def bench_step(args, dev):
    import dpvo_amd.ba
    import dpvo_amd.net

    N, H, W = args.frames, args.height, args.width
    g = torch.Generator().manual_seed(3)
    net = VONet(dtype=torch.float32, differentiable=True)
    Pf, Pi = encoder_ref.formula_params(128, "instance"), encoder_ref.formula_params(384, "none")
    net.patchify.fnet.load_state_dict({k: torch.as_tensor(v) for k, v in Pf.items()})
    net.patchify.inet.load_state_dict({k: torch.as_tensor(v) for k, v in Pi.items()})
    net.update.load_state_dict({k: torch.from_numpy(v)
                                for k, v in update_ref.formula_params(net.update.corr_dim).items()})
    net = net.to(dev)
    images = (255 * torch.rand(1, N, 3, H, W, generator=g)).to(dev)
    disps = (0.5 + torch.rand(1, N, H, W, generator=g)).to(dev)
    poses, _, _ = scene(N, 1, 8, 8, dev)
    intr = torch.tensor([W / 2.0, W / 2.0, W / 2.0, H / 2.0]).expand(1, N, 4).to(dev)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-9, weight_decay=1e-6)

    def step():
        return training.train_step(net, opt, images, SE3(poses), disps, intr, steps=args.steps,
                                   edge_drop=0, corr_dropout=1)

    for _ in range(2):
        loss, _ = step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.step_reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    out = {"bench": "train_step", "frames": N, "H": H, "W": W, "steps": args.steps,
           "loss": float(loss), "wall_ms_median": round(ts[len(ts) // 2], 2),
           "wall_ms_min": round(ts[0], 2), "wall_ms_max": round(ts[-1], 2)}
    print(json.dumps(out), flush=True)

    # the split: device time of the kernels launched under each component's
    # forward range and under each component's autograd node, one profiled step
    from torch.profiler import ProfilerActivity, profile

    undo = [labelled(net.patchify, "forward", FWD["encoders"]),
            labelled(dpvo_amd.net.CorrBlock, "__call__", FWD["corr"]),
            labelled(net.update, "forward", FWD["update"]),
            labelled(dpvo_amd.ba, "BA", FWD["BA"]),
            labelled(pops, "transform_fused", FWD["transform"]),
            labelled(training, "flow_loss", FWD["losses"]),
            labelled(training, "pose_loss", FWD["losses"])]
    try:
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
    finally:
        for u in undo:
            u()
    fwd = {k: 0.0 for k in FWD}
    bwd = {k: 0.0 for k in FWD}
    total = 0.0
    labels = {v: k for k, v in FWD.items()}
    node = "autograd::engine::evaluate_function: "
    for e in prof.events():
        if "DeviceType.CUDA" in str(getattr(e, "device_type", "")):
            total += device_us(e)  # a kernel or a copy on the device
            continue
        if e.name in labels and not any(p.name in labels for p in ancestors(e)):
            fwd[labels[e.name]] += device_us(e)
        elif e.name.startswith(node) and e.name[len(node):] in BWD:
            bwd[BWD[e.name[len(node):]]] += device_us(e)
    named = sum(fwd.values()) + sum(bwd.values())
    print(json.dumps({"bench": "train_step_split", "unit": "ms of device time, one step",
                      "forward": {k: round(v / 1e3, 2) for k, v in fwd.items()},
                      "backward": {k: round(v / 1e3, 2) for k, v in bwd.items()},
                      "rest": round((total - named) / 1e3, 2),
                      "device_total": round(total / 1e3, 2)}), flush=True)


def ancestors(e):
    p = getattr(e, "cpu_parent", None)
    while p is not None:
        yield p
        p = getattr(p, "cpu_parent", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--steps", type=int, default=18)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_step_bench: needs the GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    bench_transform(args, dev)
    bench_losses(args, dev)
    if not args.skip_step:
        bench_step(args, dev)


if __name__ == "__main__":
    main()
