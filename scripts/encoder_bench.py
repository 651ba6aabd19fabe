#!/usr/bin/env python3
"""Time the HIP feature encoders against the same arithmetic in PyTorch-ROCm.

    python scripts/encoder_bench.py [--out FILE] [--sizes 480x640 480x752] [--iters 200]

Per (image size, encoder): fnet (128, instance norm) and inet (384, no norm),
one image.  Contenders, alternating inside one process: the HIP encoder with
fp16 and with fp32 weights (dpvo_encoder.forward), and a plain PyTorch module
of the same layers (Conv2d / InstanceNorm2d / ReLU, result / 4) in fp32 and in
.half(), each eager and under hipGraph replay (the fair baseline: no launch
overhead).  Device events around `iters` calls after a warm-up, median of
`reps` windows.  Also printed: launches per call, the matrix floors (FLOPs
over the dense fp16 rate 2.5 PF/s and the exact-fp32 matrix rate 157 TF/s) and
the HBM floor (image in, map out, weights; 8 TB/s), all computed from the
shapes, and the largest difference between the HIP and PyTorch outputs.
Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import encoder_ref  # noqa: E402

PEAK_F16, PEAK_F32, PEAK_HBM = 2.5e15, 157e12, 8e12
LAUNCHES = {"instance": 25, "none": 11}


class TorchBlock(nn.Module):
    def __init__(self, cin, cout, stride, norm):
        super().__init__()
        mk = (lambda c: nn.InstanceNorm2d(c)) if norm == "instance" else (lambda c: nn.Identity())
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.norm1, self.norm2 = mk(cout), mk(cout)
        self.downsample = None
        if stride != 1:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride), mk(cout))

    def forward(self, x):
        y = torch.relu(self.norm1(self.conv1(x)))
        y = torch.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return torch.relu(x + y)


class TorchEncoder(nn.Module):
    """The encoder in plain PyTorch ops, parameter names as in the reference."""

    def __init__(self, out_dim, norm):
        super().__init__()
        self.norm1 = nn.InstanceNorm2d(32) if norm == "instance" else nn.Identity()
        self.conv1 = nn.Conv2d(3, 32, 7, stride=2, padding=3)
        self.layer1 = nn.Sequential(TorchBlock(32, 32, 1, norm), TorchBlock(32, 32, 1, norm))
        self.layer2 = nn.Sequential(TorchBlock(32, 64, 2, norm), TorchBlock(64, 64, 1, norm))
        self.conv2 = nn.Conv2d(64, out_dim, 1)

    def forward(self, x):
        x = torch.relu(self.norm1(self.conv1(x)))
        return self.conv2(self.layer2(self.layer1(x))) / 4.0


def floors(out_dim, H, W):
    """FLOPs and compulsory HBM bytes of one image, from the shapes."""
    H1, W1 = encoder_ref.out_size(H), encoder_ref.out_size(W)
    H2, W2 = encoder_ref.out_size(H1), encoder_ref.out_size(W1)
    flop, wbytes = 0.0, 0
    for i, (co, ci, k) in enumerate(encoder_ref.conv_shapes(out_dim)):
        pix = H1 * W1 if i <= 4 else H2 * W2
        flop += 2.0 * pix * co * ci * k * k
        wbytes += co * ci * k * k
    bytes_ = 4 * (3 * H * W + out_dim * H2 * W2)
    return flop, bytes_, wbytes


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def bench_cell(dev, H, W, norm, out_dim, iters, reps):
    from dpvo_amd.extractor import BasicEncoder4

    P = {k: torch.as_tensor(v) for k, v in encoder_ref.formula_params(out_dim, norm).items()}
    g = torch.Generator().manual_seed(H + W)
    img = (2 * torch.rand(1, 1, 3, H, W, generator=g) - 1).to(dev)
    variants, outs = {}, {}
    with torch.no_grad():
        for name, dt in (("hip_f16", torch.float16), ("hip_f32", torch.float32)):
            enc = BasicEncoder4(out_dim, norm, dt)
            enc.load_state_dict(P)
            enc = enc.to(dev)
            outs[name] = enc(img)[0].clone()
            variants[name] = (lambda e=enc: e(img))
        for name, dt in (("torch_f32", torch.float32), ("torch_f16", torch.float16)):
            mod = TorchEncoder(out_dim, norm)
            mod.load_state_dict(P)
            mod = mod.to(dev, dt).eval()
            x = img[0].to(dt)
            for _ in range(3):
                outs[name] = mod(x).float()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                mod(x)
            variants[name + "_eager"] = (lambda m=mod, x=x: m(x))
            variants[name + "_graph"] = gr.replay
            print(f"# {H}x{W} {norm}: {name} ready", flush=True)
        for fn in variants.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                times[k].append(window(fn, iters))
    flop, io_bytes, nweights = floors(out_dim, H, W)
    scale = float(outs["torch_f32"].abs().max())
    res = {"H": H, "W": W, "encoder": "fnet" if norm == "instance" else "inet", "norm": norm,
           "out_dim": out_dim, "flop": flop, "floor_matrix_f16_us": flop / PEAK_F16 * 1e6,
           "floor_matrix_f32_us": flop / PEAK_F32 * 1e6,
           "floor_hbm_f16_us": (io_bytes + 2 * nweights) / PEAK_HBM * 1e6,
           "floor_hbm_f32_us": (io_bytes + 4 * nweights) / PEAK_HBM * 1e6,
           "hip_launches": LAUNCHES[norm], "iters": iters, "reps": reps,
           "hip_f32_rel_diff_vs_torch_f32": float((outs["hip_f32"] - outs["torch_f32"]).abs().max()) / scale,
           "hip_f16_rel_diff_vs_torch_f32": float((outs["hip_f16"] - outs["torch_f32"]).abs().max()) / scale,
           "torch_f16_rel_diff_vs_torch_f32": float((outs["torch_f16"] - outs["torch_f32"]).abs().max()) / scale}
    for k, v in times.items():
        res[k + "_us"] = statistics.median(v)
        res[k + "_us_min_max"] = [min(v), max(v)]
    res["hip_f16_speedup_vs_torch_f16_graph"] = res["torch_f16_graph_us"] / res["hip_f16_us"]
    res["hip_f32_speedup_vs_torch_f32_graph"] = res["torch_f32_graph_us"] / res["hip_f32_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["480x640", "480x752"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("encoder_bench: needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        for norm, out_dim in (("instance", 128), ("none", 384)):
            r = bench_cell(dev, H, W, norm, out_dim, a.iters, a.reps)
            rows.append(r)
            print(json.dumps(r), flush=True)
            if a.out:  # after every cell: a later cell's failure loses nothing
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    for q in rows:
                        f.write(json.dumps(q) + "\n")
    for r in rows:
        if (r["H"], r["W"]) == (480, 640):
            # the allowance is the spread of the baseline's own windows in this run
            lo, hi = r["torch_f16_graph_us_min_max"]
            ok = r["hip_f16_us"] <= r["torch_f16_graph_us"] + (hi - lo)
            print(f"acceptance ({r['encoder']}, f16 weights, 480x640, no slower than graph-replayed "
                  f"PyTorch .half()): {'PASS' if ok else 'FAIL'} "
                  f"({r['hip_f16_us']:.1f} vs {r['torch_f16_graph_us']:.1f} us)")


if __name__ == "__main__":
    main()
