"""Call times of the two kernels of the long-term loop closure next to the
torch compositions they replace, on the GPU (device events around `reps`
calls, after a warm-up; the two versions alternate over `rounds` rounds and
the median round is reported with the spread).

    python scripts/long_term_bench.py [--reps 200] [--rounds 7] [--out FILE]

match_descriptors at 2048 x 2048 x 128 (unit-norm Gaussian descriptors, 200
planted correspondences) against `a @ b.T`, two `topk(2)` and the masks;
triangulate_tracks at 2048 tracks, M = 80, against the mini patch graph +
fastba.BA(t0 = t1 = 3, 6 iterations) + fastba.reproject of long_term.py:108-136.
Prints one JSON line; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def match_torch(a, b, ratio=0.8, max_dist=0.6):
    r2, md2 = ratio * ratio, max_dist * max_dist
    sim = a @ b.T
    d2 = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * sim).clamp_(min=0)
    rv, rj = torch.topk(d2, 2, dim=1, largest=False)
    cv, ci = torch.topk(d2, 2, dim=0, largest=False)
    rok = (rv[:, 0] <= r2 * rv[:, 1]) & (rv[:, 0] <= md2)
    cok = (cv[0] <= r2 * cv[1]) & (cv[0] <= md2)
    ar0 = torch.arange(a.shape[0], device=a.device)
    ar1 = torch.arange(b.shape[0], device=a.device)
    m0 = rok & cok[rj[:, 0]] & (ci[0][rj[:, 0]] == ar0)
    m1 = cok & rok[ci[0]] & (rj[:, 0][ci[0]] == ar1)
    return torch.where(m0, rj[:, 0], -1), torch.where(m1, ci[0], -1)


def tri_torch(D):
    """long_term.py:93-136 with the ops this tree had before the fused kernel."""
    from dpvo_amd import fastba

    dev = D["poses"].device
    track = torch.nonzero((D["m10"] >= 0) & (D["m12"] >= 0))[:, 0]
    n = track.numel()
    kps0, kps1, kps2 = D["kps0"][D["m10"][track]], D["kps1"][track], D["kps2"][D["m12"][track]]
    kk = torch.arange(n, device=dev).repeat(2)
    ii = torch.ones(2 * n, device=dev, dtype=torch.long)
    jj = torch.zeros(2 * n, device=dev, dtype=torch.long)
    jj[n:] = 2
    patches = torch.cat([kps1, D["disps"].median().expand(n, 1)], dim=-1)
    patches = patches.view(n, 3, 1, 1).expand(n, 3, 3, 3).contiguous()
    target = torch.cat([kps0, kps2])[None].contiguous()
    weight = torch.ones_like(target)
    poses, intrinsics = D["poses"].clone(), D["intrinsics"].clone()
    fastba.BA(poses, patches, intrinsics, target, weight, torch.as_tensor([1e-3], device=dev), ii,
              jj, kk, 3, 3, M=-1, iterations=6)
    coords = fastba.reproject(poses, patches, intrinsics, ii, jj, kk)[0, :, :, 1, 1]
    residual = (coords - target[0]).norm(dim=-1)
    residual = torch.maximum(residual[:n], residual[n:])
    K = intrinsics[1]
    d = patches[:, 2, 1, 1]
    pts = torch.stack([(kps1[:, 0] - K[2]) / K[0], (kps1[:, 1] - K[3]) / K[1],
                       torch.ones_like(d)], 1) / d[:, None]
    keep = (residual < 2) & (pts[:, 2] < 20)
    return pts, keep


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps  # microseconds per call


def compare(name, fused, composed, reps, rounds):
    for fn in (fused, composed):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(rounds):
        tf.append(timed(fused, reps))
        tc.append(timed(composed, reps))
    return {f"{name}_fused_us": round(statistics.median(tf), 2),
            f"{name}_fused_us_min_max": [round(min(tf), 2), round(max(tf), 2)],
            f"{name}_torch_us": round(statistics.median(tc), 2),
            f"{name}_torch_us_min_max": [round(min(tc), 2), round(max(tc), 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_term_bench: needs a GPU")
    from dpvo_amd.long_term import match_descriptors, triangulate_tracks
    from test_match_gpu import random_case
    import triangulate_ref as TR

    dev = torch.device("cuda:0")
    a, b = (torch.from_numpy(x).to(dev) for x in random_case(2048, 2048, 128, 200, 0))
    got = match_descriptors(a, b, 0.8, 0.6)
    p0, p1 = match_torch(a, b)
    res = {"match_agree": float((got.partner0 == p0).float().mean()),
           "match_count": int(got.count)}
    res.update(compare("match", lambda: match_descriptors(a, b, 0.8, 0.6),
                       lambda: match_torch(a, b), args.reps, args.rounds))

    S = TR.scene(2048, 80)
    S.m10[S.m10 >= S.kps0.shape[0]] = -1  # the composition has no range check
    D = {k: torch.from_numpy(np.ascontiguousarray(getattr(S, k))).to(dev)
         for k in ("poses", "intrinsics", "disps", "kps0", "kps1", "kps2", "m10", "m12")}
    print(json.dumps(res), flush=True)
    out = triangulate_tracks(**D)
    from dpvo_amd import fastba

    try:
        pts, keep = tri_torch(D)
        fastba.cuda_ba.check_status(D["poses"])  # the BA reports its status on a later call
        res["tri_torch_path"] = "auto"
    except RuntimeError as e:  # the automatic choice refuses this many structure-only edges
        res["tri_torch_path"] = "multi-kernel (auto: " + str(e).split(";")[0][-70:] + ")"
        fastba.cuda_ba.select_path(2)
        pts, keep = tri_torch(D)
        fastba.cuda_ba.check_status(D["poses"])
    res["tri_tracks"] = int(pts.shape[0])
    res["tri_keep_agree"] = float((out.keep[(D["m10"] >= 0) & (D["m12"] >= 0)] == keep).float().mean())
    res.update(compare("tri", lambda: triangulate_tracks(**D), lambda: tri_torch(D),
                       max(args.reps // 4, 1), args.rounds))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
