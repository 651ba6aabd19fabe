#!/usr/bin/env python3
"""Time the fused update operator against the same module in PyTorch-ROCm.

    python scripts/update_op_bench.py [--out FILE] [--E 2048 9850] [--iters 200]

Per (E, weight dtype): the HIP operator (dpvo_update.forward, group plan
excluded and timed on its own), the PyTorch module eager, and the PyTorch
module under hipGraph replay (the fair baseline: no launch overhead).  The
PyTorch module gets the dense group indices precomputed too (torch.unique
synchronises and cannot be captured).  Device events around `iters` calls,
after a warm-up, median of `reps` windows, the three variants alternating.
Also printed: the derived floors (FLOPs over the dense fp16 matrix rate 2.5
PF/s and over the exact-fp32 matrix rate 157 TF/s), the achieved fraction of
each, the launch count per call, and the largest difference between the two
implementations' outputs.  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import update_ref  # noqa: E402

DIM = 384
PEAK_F16, PEAK_F32 = 2.5e15, 157e12
LAUNCHES_FORWARD, LAUNCHES_PLAN = 9, 3


class TorchUpdate(torch.nn.Module):
    """The operator in plain PyTorch ops (the reference's original-DPVO branch
    with scatter softmax), dense group indices given."""

    def __init__(self, P, dtype, dev):
        super().__init__()
        self.P = {k: torch.as_tensor(v).to(dev, dtype) for k, v in P.items()}

    def lin(self, n, x):
        return F.linear(x, self.P[n + ".weight"], self.P[n + ".bias"])

    def ln(self, n, x):
        return F.layer_norm(x, (DIM,), self.P[n + ".weight"], self.P[n + ".bias"], 1e-3)

    def agg(self, n, x, inv, G):
        f, g = self.lin(n + ".f", x), self.lin(n + ".g", x)
        col = inv[:, None].expand(-1, DIM)
        gmax = torch.full((G, DIM), -float("inf"), dtype=x.dtype, device=x.device)
        gmax = gmax.scatter_reduce(0, col, g, "amax", include_self=True)
        ex = torch.exp(g - gmax[inv])
        den = torch.zeros((G, DIM), dtype=x.dtype, device=x.device).index_add_(0, inv, ex)
        y = torch.zeros((G, DIM), dtype=x.dtype, device=x.device).index_add_(0, inv, f * ex / den[inv])
        return self.lin(n + ".h", y)[inv]

    def forward(self, net, inp, corr, ix, jx, mx, mj, inv_k, Gk, inv_ij, Gij):
        t = torch.relu(self.lin("corr.0", corr))
        t = torch.relu(self.ln("corr.3", self.lin("corr.2", t)))
        x = self.ln("norm", net + inp + self.lin("corr.5", t))
        x = x + self.lin("c1.2", torch.relu(self.lin("c1.0", mx * x[ix])))
        x = x + self.lin("c2.2", torch.relu(self.lin("c2.0", mj * x[jx])))
        x = x + self.agg("agg_kk", x, inv_k, Gk)
        x = x + self.agg("agg_ij", x, inv_ij, Gij)
        for n, g in (("gru.0", "gru.1"), ("gru.2", "gru.3")):
            x = self.ln(n, x)
            x = x + torch.sigmoid(self.lin(g + ".gate.0", x)) * self.lin(
                g + ".res.2", torch.relu(self.lin(g + ".res.0", x)))
        r = torch.relu(x)
        return x, self.lin("d.1", r), torch.sigmoid(self.lin("w.1", r))


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def bench_cell(ext, dev, E, K0, wd, iters, reps, P):
    dt = torch.float16 if wd == "f16" else torch.float32
    ii, jj, kk = update_ref.dpvo_graph(E, M=96, seed=1)
    ix, jx = update_ref.neighbors_ref(kk, jj)
    net, inp, corr = (torch.as_tensor(a).to(dev) for a in update_ref.inputs(E, K0, 1))
    t = lambda a: torch.as_tensor(a).to(dev)
    ix, jx, gk, gij = t(ix), t(jx), t(kk), t(ii * 12345 + jj)
    # the HIP operator
    code = ext.F16 if wd == "f16" else ext.F32
    blob = ext.pack_weights([torch.from_numpy(P[n]) for n, _ in update_ref.param_shapes(K0)], K0,
                            code).to(dev)
    ws = torch.empty(ext.workspace_bytes(E, K0), dtype=torch.uint8, device=dev)
    out, d, w = torch.empty(E, DIM, device=dev), torch.empty(E, 2, device=dev), \
        torch.empty(E, 2, device=dev)
    ext.plan(gk, gij, ws)
    hip = lambda: ext.forward(blob, code, net, inp, corr, ix, jx, ws, out, d, w)
    plan = lambda: ext.plan(gk, gij, ws)
    # the PyTorch module, eager and captured
    mod = TorchUpdate(P, dt, dev)
    inv_k, inv_ij = (torch.unique(g, return_inverse=True)[1] for g in (gk, gij))
    Gk, Gij = int(inv_k.max()) + 1, int(inv_ij.max()) + 1
    ok = lambda i: ((i >= 0) & (i < E)).to(dt)[:, None]
    args = (net.to(dt), inp.to(dt), corr.to(dt), ix.clamp(0, E - 1), jx.clamp(0, E - 1), ok(ix),
            ok(jx), inv_k, Gk, inv_ij, Gij)
    with torch.no_grad():
        eager = lambda: mod(*args)
        for _ in range(3):
            ref = eager()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            mod(*args)
        graph = g.replay
        variants = {"hip": hip, "torch_eager": eager, "torch_graph": graph, "hip_plan": plan}
        for fn in variants.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                times[k].append(window(fn, iters))
    hip()
    torch.cuda.synchronize()
    diff = float((out.double() - ref[0].double()).abs().max() / ref[0].double().abs().max())
    flops = 2.0 * E * (K0 * DIM + 16 * DIM * DIM) + 2.0 * (Gk + Gij) * DIM * DIM
    res = {"E": E, "K0": K0, "weights": wd, "groups_kk": Gk, "groups_ij": Gij, "flop": flops,
           "floor_f16_us": flops / PEAK_F16 * 1e6, "floor_f32_us": flops / PEAK_F32 * 1e6,
           "launches_forward": LAUNCHES_FORWARD, "launches_plan": LAUNCHES_PLAN,
           "net_out_rel_diff_vs_torch": diff, "iters": iters, "reps": reps}
    for k, v in times.items():
        res[k + "_us"] = statistics.median(v)
        res[k + "_us_min_max"] = [min(v), max(v)]
    res["hip_fraction_of_f16_floor"] = res["floor_f16_us"] / res["hip_us"]
    res["hip_fraction_of_f32_floor"] = res["floor_f32_us"] / res["hip_us"]
    res["speedup_vs_torch_graph"] = res["torch_graph_us"] / res["hip_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[2048, 9850])
    ap.add_argument("--K0", type=int, default=882)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("update_op_bench: needs a GPU (no CPU path)")
    import dpvo_amd

    ext = dpvo_amd.load_extension("dpvo_update")
    dev = torch.device("cuda:0")
    P = update_ref.formula_params(a.K0)
    rows = []
    for E in a.E:
        for wd in ("f16", "f32"):
            r = bench_cell(ext, dev, E, a.K0, wd, a.iters, a.reps, P)
            rows.append(r)
            print(json.dumps(r), flush=True)
    ok = [r for r in rows if r["E"] == 9850 and r["weights"] == "f16"]
    if ok:
        print("acceptance (f16, E=9850, faster than graph-replayed PyTorch):",
              "PASS" if ok[0]["hip_us"] < ok[0]["torch_graph_us"] else "FAIL")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
