#!/usr/bin/env python3
"""Time the update operator's training forward and backward against fp32 eager
autograd of the same module in PyTorch-ROCm, in the same run.

    python scripts/update_bwd_bench.py [--out FILE] [--E 2048 9850] [--iters 20]

Per E: dpvo_update.forward_train (group plan included), dpvo_update.backward
(every gradient wanted: net, inp, corr and the 50 parameters), the device pack,
and the PyTorch module of scripts/update_op_bench.py forward plus backward
(dense group indices precomputed, as there).  Device events around `iters`
calls after a warm-up, median of `reps` windows, the variants alternating.
Also printed: the saved bytes, the launch counts, the exact-fp32 matrix floor
for three times the forward's FLOPs, and the spread of the windows.

Requirement at E = 9850: forward_train + backward <= 1.10 x the PyTorch time
(the margin is for the run-to-run spread of the two medians; a larger measured
spread between windows replaces it).  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import update_ref  # noqa: E402
from update_op_bench import DIM, PEAK_F32, TorchUpdate, window  # noqa: E402

LAUNCHES_FORWARD_TRAIN, LAUNCHES_PLAN, LAUNCHES_PACK = 10, 3, 1
LAUNCHES_BACKWARD = 144  # 3 for the plans of ix and jx, 141 for the gradients


def bench_cell(ext, dev, E, K0, iters, reps, P):
    ii, jj, kk = update_ref.dpvo_graph(E, M=96, seed=1)
    ix, jx = update_ref.neighbors_ref(kk, jj)
    net, inp, corr = (torch.as_tensor(a).to(dev) for a in update_ref.inputs(E, K0, 1))
    t = lambda a: torch.as_tensor(a).to(dev)
    ix, jx, gk, gij = t(ix), t(jx), t(kk), t(ii * 12345 + jj)
    names = [n for n, _ in update_ref.param_shapes(K0)]
    params = [torch.from_numpy(P[n]).to(dev) for n in names]
    blob = torch.empty(ext.packed_bytes(K0, ext.F32), dtype=torch.uint8, device=dev)
    ws = torch.empty(ext.workspace_bytes(E, K0), dtype=torch.uint8, device=dev)
    saved = torch.empty(ext.saved_bytes(E, K0), dtype=torch.uint8, device=dev)
    bws = torch.empty(ext.backward_workspace_bytes(E, K0), dtype=torch.uint8, device=dev)
    out = [torch.empty(E, n, device=dev) for n in (DIM, 2, 2)]
    cot = [torch.randn(E, n, device=dev) for n in (DIM, 2, 2)]
    gin = [torch.empty(E, n, device=dev) for n in (DIM, DIM, K0)]
    grads = [torch.empty_like(p) for p in params]

    def pack():
        ext.pack_weights_device(params, K0, ext.F32, blob)

    def fwd():
        ext.plan(gk, gij, ws)
        ext.forward_train(blob, net, inp, corr, ix, jx, ws, saved, *out)

    def bwd():
        ext.backward(params, saved, ix, jx, K0, cot[0], cot[1], cot[2], gin[0], gin[1], gin[2],
                     grads, bws)

    # the PyTorch module: fp32 eager autograd, forward plus backward
    mod = TorchUpdate(P, torch.float32, dev)
    for v in mod.P.values():
        v.requires_grad_()
    inv_k, inv_ij = (torch.unique(g, return_inverse=True)[1] for g in (gk, gij))
    Gk, Gij = int(inv_k.max()) + 1, int(inv_ij.max()) + 1
    ok = lambda i: ((i >= 0) & (i < E)).float()[:, None]
    tin = [a.clone().requires_grad_() for a in (net, inp, corr)]
    rest = (ix.clamp(0, E - 1), jx.clamp(0, E - 1), ok(ix), ok(jx), inv_k, Gk, inv_ij, Gij)
    leaves = tin + [mod.P[n] for n in names]

    def torch_step():
        o = mod(*tin, *rest)
        return torch.autograd.grad(o, leaves, cot)

    variants = {"pack": pack, "forward_train": fwd, "backward": bwd, "torch_fwd_bwd": torch_step}
    pack()
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    ref = torch_step()
    bwd()
    torch.cuda.synchronize()
    diff = max(float((a.double() - b.double()).abs().max() / b.double().abs().max())
               for a, b in zip(gin + grads, ref) if float(b.abs().max()) > 1e-3)
    flops = 2.0 * E * (K0 * DIM + 16 * DIM * DIM) + 2.0 * (Gk + Gij) * DIM * DIM
    res = {"E": E, "K0": K0, "saved_bytes": ext.saved_bytes(E, K0),
           "saved_bytes_per_edge": ext.saved_bytes(E, K0) / E,
           "backward_workspace_bytes": ext.backward_workspace_bytes(E, K0),
           "launches_forward_train": LAUNCHES_FORWARD_TRAIN + LAUNCHES_PLAN,
           "launches_backward": LAUNCHES_BACKWARD, "launches_pack": LAUNCHES_PACK,
           "floor_f32_3x_forward_us": 3.0 * flops / PEAK_F32 * 1e6,
           "worst_rel_diff_vs_torch": diff, "iters": iters, "reps": reps}
    for k, v in times.items():
        res[k + "_us"] = statistics.median(v)
        res[k + "_us_min_max"] = [min(v), max(v)]
    res["hip_fwd_bwd_us"] = res["forward_train_us"] + res["backward_us"]
    res["ratio_vs_torch"] = res["hip_fwd_bwd_us"] / res["torch_fwd_bwd_us"]
    spread = lambda v: (max(v) - min(v)) / statistics.median(v)
    res["window_spread"] = max(spread(times["torch_fwd_bwd"]),
                               spread([a + b for a, b in zip(times["forward_train"],
                                                             times["backward"])]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[2048, 9850])
    ap.add_argument("--K0", type=int, default=882)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("update_bwd_bench: needs a GPU (no CPU path)")
    import dpvo_amd

    ext = dpvo_amd.load_extension("dpvo_update")
    dev = torch.device("cuda:0")
    P = update_ref.formula_params(a.K0)
    rows = []
    for E in a.E:
        r = bench_cell(ext, dev, E, a.K0, a.iters, a.reps, P)
        rows.append(r)
        print(json.dumps(r), flush=True)
    for r in rows:
        if r["E"] == 9850:
            margin = max(0.10, r["window_spread"])
            print(f"requirement (E=9850, forward_train + backward <= {1 + margin:.2f} x PyTorch): "
                  f"ratio {r['ratio_vs_torch']:.2f}",
                  "PASS" if r["ratio_vs_torch"] <= 1 + margin else "FAIL")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
