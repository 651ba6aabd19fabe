"""Timing of the differentiable BA layer (dpvo_amd.ba.BA over ba_layer.hip)
against the same layer composed from the ops the project had before it:
projective_ops.transform(jacobian=True), index_add and ba.block_solve.

  training shape  15 frames x 80 patches, every patch to every frame
                  (E = 18000), fixedp = 1, ep = 10, fp32: forward + backward
  live shape      synthetic.make_dpvo_window() (22 frames x 96 patches,
                  E = 37824), fixedp = n - 10, ep = 100, fp32: forward only

HIP events, warm-up, medians; kernel launches counted with torch.profiler.

    python scripts/ba_layer_bench.py [--reps 30]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import dpvo_amd  # noqa: E402,F401
from dpvo_amd import projective_ops as pops  # noqa: E402
from dpvo_amd.ba import BA, block_solve  # noqa: E402
from dpvo_amd.lietorch import SE3  # noqa: E402
from dpvo_amd.synthetic import make_dpvo_window, make_graph, reproject_centres  # noqa: E402


def composed(poses, patches, intrinsics, targets, weights, lmbda, ii, jj, kk, bounds, ep, fixedp, n):
    """The layer from separate ops (B = 1), every patch index kept (m = M)."""
    M = patches.shape[1]
    coords, v, (Ji, Jj, Jz) = pops.transform(poses, patches, intrinsics, ii, jj, kk, jacobian=True)
    p = coords.shape[3]
    c = coords[..., p // 2, p // 2, :]
    r = targets - c
    v = v.to(r.dtype) * (r.norm(dim=-1) < 250).to(r.dtype)
    v = v * ((c[..., 0] > bounds[0]) & (c[..., 1] > bounds[1]) & (c[..., 0] < bounds[2]) &
             (c[..., 1] < bounds[3])).to(r.dtype)
    r = (v[..., None] * r).unsqueeze(-1)
    w = (v[..., None] * weights).unsqueeze(-1)
    wJi, wJj, wJz = (w * Ji).transpose(2, 3), (w * Jj).transpose(2, 3), (w * Jz).transpose(2, 3)
    nf = n - fixedp
    fi, fj = ii - fixedp, jj - fixedp

    def mat(blocks, a, b, cols):
        ok = (a >= 0) & (b >= 0)
        idx = torch.where(ok, a * cols + b, torch.zeros_like(a))
        out = blocks.new_zeros((1, nf * cols) + blocks.shape[2:])
        return out.index_add_(1, idx, blocks * ok.view(1, -1, 1, 1).to(blocks.dtype))

    def vec(vals, a, rows):
        ok = a >= 0
        idx = torch.where(ok, a, torch.zeros_like(a))
        out = vals.new_zeros((1, rows) + vals.shape[2:])
        return out.index_add_(1, idx, vals * ok.view(1, -1, 1, 1).to(vals.dtype))

    B = (mat(wJi @ Ji, fi, fi, nf) + mat(wJi @ Jj, fi, fj, nf) + mat(wJj @ Ji, fj, fi, nf) +
         mat(wJj @ Jj, fj, fj, nf)).view(1, nf, nf, 6, 6)
    E = (mat(wJi @ Jz, fi, kk, M) + mat(wJj @ Jz, fj, kk, M)).view(1, nf, M, 6, 1)
    C = vec(wJz @ Jz, kk, M)
    vv = (vec(wJi @ r, fi, nf) + vec(wJj @ r, fj, nf)).view(1, nf, 1, 6, 1)
    u = vec(wJz @ r, kk, M)
    Q = 1.0 / (C + lmbda)
    EQ = E * Q[:, None]
    Ed, EQd = E[0, :, :, :, 0].permute(0, 2, 1).reshape(6 * nf, M), EQ[0, :, :, :, 0].permute(0, 2, 1).reshape(6 * nf, M)
    S = B - (EQd @ Ed.T).view(nf, 6, nf, 6).permute(0, 2, 1, 3)[None]
    y = vv - (EQd @ u.view(M, 1)).view(1, nf, 1, 6, 1)
    dX = block_solve(S, y, ep=ep, lm=1e-4)
    dZ = Q * (u - (Ed.T @ dX.reshape(6 * nf, 1)).view(1, M, 1, 1))
    x, yy, disps = patches.unbind(dim=2)
    disps = (disps + dZ.view(1, M, 1, 1)).clamp(min=1e-3, max=10.0)
    N = poses.data.shape[1]
    full = torch.nn.functional.pad(dX.view(nf, 6), (0, 0, fixedp, N - n)).view(1, N, 6)
    return poses.retr(full), torch.stack([x, yy, disps], dim=2)


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2]


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages()
                       if getattr(e, "device_type", None) is not None and "DeviceType.CUDA" in str(e.device_type)))
    except Exception as e:  # the profiler is optional: report instead of failing the timing
        return f"n/a ({type(e).__name__})"


def kernel_table(fn, top=14):
    """Device time per kernel of one call of fn (profiler averages over 5 calls)."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    rows = [(e.key[:60], e.count // 5, round(getattr(e, "device_time_total", 0.0) / 5, 1))
            for e in prof.key_averages() if "DeviceType.CUDA" in str(getattr(e, "device_type", ""))]
    return sorted(rows, key=lambda r: -r[2])[:top]


def training_graph(dev):
    G = make_graph(15, 80, 1200, seed=0)
    kk = torch.arange(1200).repeat_interleave(15)
    jj = torch.arange(15).repeat(1200)
    ii = kk // 80
    ctr = reproject_centres(G.poses.double().numpy(), G.patches.double().numpy(), (80.0, 80.0, 80.0, 60.0),
                            ii.numpy(), jj.numpy(), kk.numpy())
    g = torch.Generator().manual_seed(1)
    target = torch.from_numpy(ctr).float() + 0.5 * torch.randn(len(ii), 2, generator=g)
    weight = torch.rand(len(ii), 2, generator=g)
    t = lambda x: x.to(dev)[None]  # noqa: E731
    return dict(P=t(G.poses), K=t(G.patches), I=t(G.intrinsics), T=t(target), W=t(weight),
                ii=ii.to(dev), jj=jj.to(dev), kk=kk.to(dev), n=15, fixedp=1, ep=10.0)


def live_graph(dev):
    G = make_dpvo_window()
    t = lambda x: x.to(dev)[None]  # noqa: E731
    return dict(P=t(G.poses), K=t(G.patches), I=t(G.intrinsics), T=t(G.target), W=t(G.weight),
                ii=G.ii.to(dev), jj=G.jj.to(dev), kk=G.kk.to(dev), n=G.F, fixedp=G.F - 10, ep=100.0)


def runner(g, which, backward):
    bounds = (0.0, 0.0, 159.0, 119.0)

    def run():
        leaves = [x.detach().clone().requires_grad_(backward) for x in (g["P"], g["K"], g["T"], g["W"])]
        P, K, T, W = leaves
        with torch.set_grad_enabled(backward):
            if which == "fused":
                poses, patches = BA(SE3(P), K, g["I"], T, W, 1e-4, g["ii"], g["jj"], g["kk"], bounds,
                                    ep=g["ep"], fixedp=g["fixedp"], num_poses=g["n"])
            else:
                poses, patches = composed(SE3(P), K, g["I"], T, W, 1e-4, g["ii"], g["jj"], g["kk"],
                                          bounds, g["ep"], g["fixedp"], g["n"])
            if backward:
                (poses.data.sum() + patches.sum()).backward()
        return poses.data.detach(), patches.detach(), [x.grad for x in leaves]

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--kernels", action="store_true", help="also print the fused layer's time per kernel")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, g, backward in (("training", training_graph(dev), True), ("live", live_graph(dev), False)):
        fused, comp = runner(g, "fused", backward), runner(g, "composed", backward)
        a, b = fused(), comp()
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max())  # noqa: E731
        out = {"shape": name, "E": int(g["ii"].numel()), "M": int(g["K"].shape[1]), "n": g["n"],
               "fixedp": g["fixedp"], "backward": backward,
               "fused_us": round(timed(fused, args.reps), 1),
               "composed_us": round(timed(comp, args.reps), 1),
               "poses_rel_diff": rel(a[0], b[0]), "patches_rel_diff": rel(a[1], b[1])}
        if backward:
            out["grad_rel_diff"] = [rel(x, y) for x, y in zip(a[2], b[2])]
            # the same comparison in fp64: the fp32 composition carries fp32 atomics
            # and an fp32 Cholesky, the fused layer reduces and solves in fp64
            g64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v)
                   for k, v in g.items()}
            a64, b64 = runner(g64, "fused", True)(), runner(g64, "composed", True)()
            out["grad_rel_diff_fp64"] = [rel(x, y) for x, y in zip(a64[2], b64[2])]
        out["fused_launches"] = launches(fused)
        out["composed_launches"] = launches(comp)
        print(json.dumps(out), flush=True)
        if args.kernels:
            for row in kernel_table(fused):
                print(json.dumps({"shape": name, "kernel": row[0], "calls": row[1], "us_per_call_of_layer": row[2]}),
                      flush=True)


if __name__ == "__main__":
    main()
