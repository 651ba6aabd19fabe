#!/usr/bin/env python
"""The training loop of DPVO's train.py (44-160) on the MI355X: TartanAir from a
directory (dpvo_amd.data_readers: frame graph, sampler, augmentation and depth
normalisation on the device), AdamW, OneCycleLR, structure-only for the first
1000 steps, `train_step`, a periodic torch.save.

    python scripts/train.py --datapath datasets/TartanAir --name run0 \
        [--ckpt dpvo.pth] [--steps 240000] [--n_frames 15] [--cache graphs/]

It has not been run end to end here: the tree has no dataset and no weights.
The logger and the validation run of the reference's loop are not part of it.
"""
import argparse
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SPLIT = os.path.join(REPO, "tests", "golden", "tartan_test_split.txt")


def train(args):
    from dpvo_amd import TartanAir, VONet, train_step
    from dpvo_amd.lietorch import SE3

    db = TartanAir(args.datapath, n_frames=args.n_frames, cache=args.cache, test_split=args.test_split,
                   seed=args.seed)
    if len(db) == 0:
        sys.exit(f"train: no training scene under {args.datapath}")
    net = VONet(dtype=torch.float32, differentiable=True).cuda()
    net.train()
    if args.ckpt is not None:
        state = torch.load(args.ckpt, map_location="cuda")
        net.load_state_dict(OrderedDict((k.replace("module.", ""), v) for k, v in state.items()),
                            strict=False)
    optimizer = torch.optim.AdamW(net.parameters(), lr=args.lr, weight_decay=1e-6)
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, args.lr, args.steps, pct_start=0.01,
                                                    cycle_momentum=False, anneal_strategy="linear")
    os.makedirs(args.out, exist_ok=True)
    order_rng = np.random.default_rng(args.seed)
    total_steps = 0
    while total_steps < args.steps:
        for index in order_rng.permutation(len(db)):           # DataLoader(shuffle=True, batch_size=1)
            images, poses, disps, intrinsics = db[int(index)]
            so = total_steps < 1000 and args.ckpt is None       # poses fixed to gt for the first 1k steps
            loss, metrics = train_step(net, optimizer, images, SE3(poses).inv(), disps, intrinsics,
                                       steps=18, clip=args.clip, scheduler=scheduler,
                                       structure_only=so, M=1024)
            total_steps += 1
            if total_steps % args.log_every == 0:                # the only host reads of the loop
                print(total_steps, " ".join(f"{k} {float(v):.4f}" for k, v in metrics.items()), flush=True)
            if total_steps % args.save_every == 0 or total_steps == args.steps:
                torch.save(net.state_dict(), os.path.join(args.out, "%s_%06d.pth" % (args.name, total_steps)))
            if total_steps >= args.steps:
                break


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="bla", help="name your experiment")
    ap.add_argument("--datapath", default="datasets/TartanAir")
    ap.add_argument("--ckpt", help="checkpoint to restore")
    ap.add_argument("--steps", type=int, default=240000)
    ap.add_argument("--lr", type=float, default=0.00008)
    ap.add_argument("--clip", type=float, default=10.0)
    ap.add_argument("--n_frames", type=int, default=15)
    ap.add_argument("--cache", default="graph_cache", help="directory of the per-scene frame graphs")
    ap.add_argument("--test_split", default=SPLIT, help="file of held-out scene names")
    ap.add_argument("--out", default="checkpoints")
    ap.add_argument("--save_every", type=int, default=10000)
    ap.add_argument("--log_every", type=int, default=100)
    ap.add_argument("--seed", type=int, default=None)
    train(ap.parse_args())
