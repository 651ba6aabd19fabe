#!/usr/bin/env python
"""Times of the image-stream front (frame_prepare) and the evaluation back
(trajectory_ate) on the device.

    python scripts/stream_bench.py [--iters 2000] [--json out.json]

  frame_prepare   480 x 752 grey, EuRoC's calibration, scale 1
                  1080 x 1920 x 3, iphone's calibration, scale 0.5
                  beside each: a device-to-device copy of the same output bytes
  trajectory_ate  n = m = 4096

Device events around `iters` back-to-back calls on one stream after a warm-up
of the same shape; the figure is the mean per call, host enqueue included
where it is the longer of the two.  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLDEN = os.path.join(REPO, "tests", "golden")


def timed(fn, iters, warmup=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_bench: needs a GPU")
    from dpvo_amd.evaluation import ate
    from dpvo_amd.stream import prepare_frame, read_calib

    import ate_ref

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    for name, shape, calib, scale in (
            ("euroc_480x752_grey", (480, 752), "calib_euroc.txt", 1.0),
            ("iphone_1080x1920x3_half", (1080, 1920, 3), "calib_iphone.txt", 0.5)):
        calib = read_calib(os.path.join(GOLDEN, calib))
        raw = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev)
        image, _ = prepare_frame(raw, calib, scale)
        buf, dst = torch.empty_like(image), torch.empty_like(image)
        t_prep = timed(lambda: prepare_frame(raw, calib, scale, out=buf), args.iters)
        t_copy = timed(lambda: dst.copy_(buf), args.iters)
        out[name] = {"out_shape": list(image.shape), "out_bytes": image.numel(),
                     "frame_prepare_us": round(t_prep, 2), "d2d_copy_same_bytes_us": round(t_copy, 2)}
        print(name, out[name], flush=True)
    ex, et, rx, rt = ate_ref.make_case(4096, 4096, 0)
    ex, et, rx, rt = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (ex, et, rx, rt))
    r = ate(ex, et, rx, rt)
    out["trajectory_ate_4096"] = {"pairs": int(r.stats[7].item()), "status": int(r.status.item()),
                                  "trajectory_ate_us": round(timed(lambda: ate(ex, et, rx, rt),
                                                                   max(args.iters // 4, 1)), 2)}
    print("trajectory_ate_4096", out["trajectory_ate_4096"], flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
