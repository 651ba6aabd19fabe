#!/usr/bin/env python
"""Track a sequence as it sits on disk and score it against a ground truth:
the body of evaluate_euroc.py's run() plus its scoring (:103-119), without cv2,
a reader process or evo.

    python scripts/evaluate_sequence.py --imagedir DIR --calib calib.txt \
        --groundtruth gt.txt --network dpvo.pth [--stride 2] [--skip 0] [--scale 1.0] \
        [--save_trajectory out.txt]

Frames are the sorted *.png / *.jpeg / *.jpg of --imagedir; a frame's timestamp
is its file name without the extension, times --stamp_scale (as
evaluate_euroc.py:106 reads it).  --groundtruth is a TUM file
`t x y z qx qy qz qw` in the same unit.  Prints the ATE RMSE after Sim(3)
alignment (evo's ape with align=True, correct_scale=True).

Not exercised end to end in this repository: neither the trained weights
(dpvo.pth) nor any dataset ships with it.  Its parts are tested one by one
(tests/test_stream_*.py, tests/test_evaluate_*.py, tests/test_tracker_gpu.py).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--imagedir", required=True)
    ap.add_argument("--calib", required=True)
    ap.add_argument("--groundtruth", required=True)
    ap.add_argument("--network", required=True)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--skip", type=int, default=0)
    ap.add_argument("--scale", type=float, default=1.0, choices=[1.0, 0.5])
    ap.add_argument("--stamp_scale", type=float, default=1.0,
                    help="file-name stamp -> ground-truth unit (1e-9 for EuRoC's nanoseconds "
                         "against a ground truth in seconds)")
    ap.add_argument("--max_diff", type=float, default=0.01)
    ap.add_argument("--swap_rb", action="store_true",
                    help="feed colour frames as BGR, the order cv2.imread gives the reference")
    ap.add_argument("--save_trajectory")
    args = ap.parse_args()

    from dpvo_amd import DPVO, ImageStream, ate, default_config, read_tum, write_tum

    stream = ImageStream(args.imagedir, args.calib, stride=args.stride, skip=args.skip,
                         scale=args.scale, swap_rb=args.swap_rb)
    if len(stream) == 0:
        sys.exit(f"no images in {args.imagedir}")
    stamps = np.array([float(p.stem) for p in stream.files]) * args.stamp_scale
    ref_t, ref_poses = read_tum(args.groundtruth)

    slam = None
    with torch.no_grad():
        for t, image, intrinsics in stream:
            if slam is None:
                slam = DPVO(default_config(), args.network, ht=image.shape[1], wd=image.shape[2])
            slam(t, image, intrinsics)
        poses, _ = slam.terminate()

    poses = torch.as_tensor(poses)
    if not poses.is_cuda:
        poses = poses.cuda()
    result = ate(poses, stamps, ref_poses[:, :3], ref_t, max_diff=args.max_diff)
    stats, status = result.stats.cpu().numpy(), int(result.status.item())  # the one host read
    if args.save_trajectory:
        write_tum(args.save_trajectory, poses, stamps)
    if status:
        sys.exit(f"ATE not available: status {status} (1: fewer than 3 matched stamps, "
                 f"2: degenerate alignment, 4: unsorted stamps), {int(stats[7])} pairs")
    print(f"pairs {int(stats[7])}  ATE rmse {stats[0]:.6f}  mean {stats[1]:.6f}  "
          f"median {stats[2]:.6f}  std {stats[3]:.6f}  min {stats[4]:.6f}  max {stats[5]:.6f}")


if __name__ == "__main__":
    main()
