#!/usr/bin/env python
"""Times of the training data kernels (csrc/dataset.hip) beside the reference's
own formulation on the same device.

    python scripts/dataset_bench.py [--reps 15] [--json out.json]

  frame_distance_matrix   N = 1000 frames of 30 x 40 points, against
                          dpvo_amd.projective_ops.transform on P = 1 patches in
                          chunks of 2048 pairs with the per-chunk host copy
                          (rgbd_utils.compute_distance_matrix_flow's loop)
  RGBDAugmentor           8 x 480 x 640, crop 480 x 640, colour and scale 1.3,
                          against F.interpolate (bicubic / nearest) and the slice
                          -- the spatial part alone: the reference's colour path
                          runs in PIL on the host
  normalize_depth         8 x 480 x 640 against torch.quantile

Every figure is the median of `reps` runs, each between two device events,
after a warm-up run of the same shape; the composition's host copies are inside
its events because they are part of it.  Needs a GPU: there is no CPU path.
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


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def composed_distance(poses, disps, intrinsics):
    """compute_distance_matrix_flow with the flow through transform(.., valid=True)."""
    from dpvo_amd import projective_ops as pops
    from dpvo_amd.lietorch import SE3

    N, h, w = disps.shape
    G = SE3(poses[None]).inv()
    y, x = torch.meshgrid(torch.arange(h, device=poses.device).float(),
                          torch.arange(w, device=poses.device).float(), indexing="ij")
    # one P = 1 patch per grid point of every frame: [1, N h w, 3, 1, 1]
    patches = torch.stack([x.expand(N, h, w), y.expand(N, h, w), disps], -1).view(1, N * h * w, 3, 1, 1)
    xy = torch.stack([x, y], -1).view(1, 1, h * w, 2)
    pts = torch.arange(h * w, device=poses.device)
    ii, jj = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    ii, jj = ii.reshape(-1).to(poses.device), jj.reshape(-1).to(poses.device)
    matrix = np.zeros((N, N), dtype=np.float32)
    K = intrinsics[None]

    def induced(a, b):
        src = a.repeat_interleave(h * w)
        dst = b.repeat_interleave(h * w)
        kk = src * (h * w) + pts.repeat(a.numel())
        x1, val = pops.transform(G, patches, K, src, dst, kk, valid=True)
        return x1.view(1, a.numel(), h * w, 2) - xy, val.view(1, a.numel(), h * w)

    s = 2048
    for i in range(0, ii.shape[0], s):
        flow1, val1 = induced(ii[i:i + s], jj[i:i + s])
        flow2, val2 = induced(jj[i:i + s], ii[i:i + s])
        flow = torch.stack([flow1, flow2], dim=2)
        val = torch.stack([val1, val2], dim=2)
        mag = flow.norm(dim=-1).clamp(max=100.0)
        mag = mag.view(mag.shape[1], -1)
        val = val.view(val.shape[1], -1)
        mag = (mag * val).mean(-1) / val.mean(-1)
        mag[val.mean(-1) < 0.7] = np.inf
        matrix[ii[i:i + s].cpu().numpy(), jj[i:i + s].cpu().numpy()] = mag.cpu().numpy()
    return matrix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dataset_bench: needs a GPU")
    from dpvo_amd import data_readers as dr

    import dataset_ref

    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps}

    N = args.frames
    poses, disps, K, _ = dataset_ref.make_scene(N, 30, 40, 0)
    poses, disps, K = (torch.from_numpy(a).to(dev) for a in (poses, disps, K))
    D = dr.frame_distance_matrix(poses, disps, K).cpu().numpy()
    t_k = median_ms(lambda: dr.frame_distance_matrix(poses, disps, K), args.reps)
    ref = composed_distance(poses, disps, K)
    fin = np.isfinite(ref) & np.isfinite(D)
    t_c = median_ms(lambda: composed_distance(poses, disps, K), max(args.reps // 5, 3), warmup=0)  # `ref` above was its warm-up
    out["frame_distance_matrix"] = {
        "N": N, "points": [30, 40], "kernel_ms": round(t_k[0], 3), "kernel_min_max_ms": [round(v, 3) for v in t_k[1:]],
        "composition_ms": round(t_c[0], 2), "composition_min_max_ms": [round(v, 2) for v in t_c[1:]],
        "ratio": round(t_c[0] / t_k[0], 1),
        "inf_pattern_differs": int((np.isinf(ref) != np.isinf(D)).sum()),
        "max_rel_diff_fp32_composition": float(np.max(np.abs(ref[fin] - D[fin]) / np.maximum(np.abs(D[fin]), 1e-3)))}
    print("frame_distance_matrix", out["frame_distance_matrix"], flush=True)
    t_g = median_ms(lambda: dr.build_frame_graph(poses, disps, K), args.reps)
    out["build_frame_graph_ms"] = round(t_g[0], 3)
    print("build_frame_graph_ms", out["build_frame_graph_ms"], flush=True)

    g = torch.Generator().manual_seed(0)
    images = (torch.rand(8, 3, 480, 640, generator=g) * 255).to(dev)
    depth = (torch.rand(8, 480, 640, generator=g) + 0.1).to(dev)
    intr = torch.tensor([[320.0, 320.0, 320.0, 240.0]]).repeat(8, 1).to(dev)
    pose8 = torch.rand(8, 7, generator=g).to(dev)
    aug = dr.RGBDAugmentor((480, 640))
    s = 1.3
    full = dr.AugmentParams(do_color=True, order=(2, 1, 3, 0), brightness=1.2, contrast=0.8,
                            saturation=1.3, hue=0.04, scale=s)
    only = dr.AugmentParams(do_color=False, scale=s)

    def composed_spatial():
        ht1, wd1 = int(s * 480), int(s * 640)
        y0, x0 = (ht1 - 480) // 2, (wd1 - 640) // 2
        a = F.interpolate(images, (ht1, wd1), mode="bicubic", align_corners=False)
        b = F.interpolate(depth[:, None], (ht1, wd1))
        k = s * intr - torch.tensor([0.0, 0.0, x0, y0], device=dev)
        return (a[:, :, y0:y0 + 480, x0:x0 + 640].contiguous(),
                b[:, 0, y0:y0 + 480, x0:x0 + 640].contiguous(), k)

    t_sp = median_ms(lambda: aug(images, pose8, depth, intr, params=only), args.reps)
    t_full = median_ms(lambda: aug(images, pose8, depth, intr, params=full), args.reps)
    t_ref = median_ms(composed_spatial, args.reps)
    out["augment_8x480x640"] = {"scale": s, "spatial_kernel_ms": round(t_sp[0], 3),
                                "colour_and_spatial_kernels_ms": round(t_full[0], 3),
                                "interpolate_and_slice_ms": round(t_ref[0], 3),
                                "ratio_spatial": round(t_ref[0] / t_sp[0], 2)}
    print("augment_8x480x640", out["augment_8x480x640"], flush=True)

    t_n = median_ms(lambda: dr.normalize_depth(depth, pose8), args.reps)
    t_q = median_ms(lambda: (depth / (0.7 * torch.quantile(depth, 0.98)), pose8), args.reps)
    out["normalize_depth_8x480x640"] = {"kernel_ms": round(t_n[0], 3), "torch_quantile_ms": round(t_q[0], 3)}
    print("normalize_depth_8x480x640", out["normalize_depth_8x480x640"], flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
