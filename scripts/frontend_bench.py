"""Timing of the frame front-end and the trajectory read-out
(dpvo_amd/frontend.py) against the chains of generic calls they replace, on
the same data and in the same process.

init_frame, M in {80, 96}, P = 3, n = 20: one launch, against the head of
DPVO.__call__ as the reference writes it (dpvo.py:931-965) on this package's
lietorch: SE3 inv / mul / log / exp / mul on fp32 tensors, torch.median over
the depths of the last three frames, and the row copies.  Neither side
synchronises with the host.

trajectory, counter = 4096 (the reference's BUFFER_SIZE), 10 % keyframes,
chains of depth 1 to 4: 2 + 12 launches, against terminate's Python recursion
(dpvo.py:385-411) over lietorch.SE3 on the same poses and records, up to the
stacked and inverted poses on the device.

Device times: medians of HIP-event timings around the whole Python call after
warm-up.  The two sides of each comparison alternate inside one loop.  A third
figure takes the host's enqueue out of the new call: many calls captured in one
graph, the replay time divided by their number.  Each case runs in a child
process under its own time limit.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT = 240  # seconds per case


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _alternate(f_new, f_old, reps, warmup):
    for _ in range(warmup):
        f_new()
        f_old()
    t_new, t_old = [], []
    for _ in range(reps):
        t_new.append(_timed(f_new))
        t_old.append(_timed(f_old))
    return _median(t_new), _median(t_old), min(t_new), min(t_old)


def _graph_ms(fn, calls, reps=20):
    """Device time per call with the host's enqueue taken out: `calls` calls
    captured in one graph, the graph replayed; median replay time / calls."""
    import torch

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm on a side stream, as capture needs
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return _median([_timed(g.replay) for _ in range(reps)]) / calls


def _track(N, seed):
    """a smooth camera track [N, 7] fp32"""
    import torch

    from dpvo_amd.lietorch import SE3

    g = torch.Generator().manual_seed(seed)
    xi = torch.cat([0.05 * torch.randn(N, 3, generator=g), 0.02 * torch.randn(N, 3, generator=g)],
                   -1).cuda()
    P = SE3.exp(xi[0:1])
    rows = [P.data[0]]
    for f in range(1, N):
        P = SE3.exp(xi[f:f + 1]) * P
        rows.append(P.data[0])
    return torch.stack(rows)


def run_init(M):
    sys.path.insert(0, ROOT)
    import torch

    from dpvo_amd import frontend
    from dpvo_amd.lietorch import SE3

    dev = torch.device("cuda:0")
    N, P, n, counter, RES, damping = 36, 3, 20, 25, 4.0, 0.5
    g = torch.Generator().manual_seed(M)
    poses = _track(N, 1)
    patches = (torch.rand(N * M, 3, P, P, generator=g) + 0.1).to(dev)
    intrinsics = torch.rand(N, 4, generator=g).to(dev) * 100
    tstamps = torch.zeros(N, dtype=torch.long, device=dev)
    tlist = [0.1 * i for i in range(counter + 1)]
    times = torch.tensor(tlist + [0.0] * 8, dtype=torch.float64, device=dev)
    new_patches = (torch.rand(1, M, 3, P, P, generator=g) + 0.1).to(dev)
    new_intr = torch.tensor([517.3, 516.5, 318.6, 255.3], device=dev)
    patches_ = patches.view(N, M, 3, P, P)

    def new():
        frontend.init_frame(poses, patches, intrinsics, tstamps, times, new_patches, new_intr, n,
                            counter, M, damping=damping, res=RES)

    def old():  # dpvo.py:933-965, line by line
        tstamps[n] = counter
        intrinsics[n] = new_intr / RES
        P1 = SE3(poses[n - 1])
        P2 = SE3(poses[n - 2])
        *_, a, b, c = [1] * 3 + tlist
        fac = (c - b) / (b - a)
        xi = damping * fac * (P1 * P2.inv()).log()
        poses[n] = (SE3.exp(xi) * P1).data
        s = torch.median(patches_[n - 3:n, :, 2])
        new_patches[:, :, 2] = s
        patches_[n] = new_patches[0]

    new()
    got = (poses[n].clone(), patches_[n].clone(), intrinsics[n].clone())
    old()
    assert torch.equal(got[1], patches_[n]) and torch.equal(got[2], intrinsics[n])
    dpose = (got[0] - poses[n]).abs().max().item()  # fp64 kernel against the fp32 chain
    t_new, t_old, m_new, m_old = _alternate(new, old, reps=200, warmup=20)
    print(f"init_frame M={M} P={P} n={n}: patches / intrinsics equal the chain's bit for bit, "
          f"pose max abs difference {dpose:.1e}", flush=True)
    print(f"  frontend.init_frame (1 launch):                    median {1e3 * t_new:8.1f} us"
          f"   min {1e3 * m_new:8.1f} us", flush=True)
    print(f"  lietorch + torch.median + row copies (reference):  median {1e3 * t_old:8.1f} us"
          f"   min {1e3 * m_old:8.1f} us", flush=True)
    print(f"  replayed from a graph of 50 calls, per call:       {1e3 * _graph_ms(new, 50):8.1f} us",
          flush=True)


def run_trajectory(counter):
    sys.path.insert(0, ROOT)
    import torch

    from dpvo_amd import frontend, lietorch
    from dpvo_amd.lietorch import SE3

    dev = torch.device("cuda:0")
    kfs = list(range(0, counter, 10))  # 10 % keyframes
    n = len(kfs)
    poses = _track(n, 2)
    tstamps = torch.tensor(kfs, dtype=torch.long, device=dev)
    pairs = []
    for t in range(counter):
        j = t % 10
        if j:  # depths 1 2 3 4 | 1 2 3 4 | 1 behind keyframe 10 k
            pairs.append((t, t - j if j in (5, 9) else t - 1))
    g = torch.Generator().manual_seed(3)
    xi = torch.cat([0.02 * torch.randn(len(pairs), 3, generator=g),
                    0.01 * torch.randn(len(pairs), 3, generator=g)], -1).to(dev)
    log = SE3.exp(xi).data.contiguous()
    delta = (log, torch.tensor(pairs, dtype=torch.long, device=dev),
             torch.tensor([len(pairs)], dtype=torch.int32, device=dev))

    def new():
        return frontend.trajectory(poses, tstamps, n, delta, counter, inverse=True)[0]

    poses_h, log_h = poses, log

    def old():  # dpvo.py:385-411
        traj = {kfs[i]: poses_h[i] for i in range(n)}
        dl = {t1: (t0, SE3(log_h[r])) for r, (t1, t0) in enumerate(pairs)}

        def get_pose(t):
            if t in traj:
                return SE3(traj[t])
            t0, dP = dl[t]
            return dP * get_pose(t0)

        ps = [get_pose(t) for t in range(counter)]
        return lietorch.stack(ps, dim=0).inv().data

    a, b = new(), old()
    sgn = torch.sign((a[:, 3:] * b[:, 3:]).sum(-1, keepdim=True))  # q and -q are one rotation
    err = (a - torch.cat([b[:, :3], sgn * b[:, 3:]], -1)).abs().max().item()
    t_new, t_old, m_new, m_old = _alternate(new, old, reps=5, warmup=1)
    t_new, _, m_new, _ = _alternate(new, lambda: None, reps=200, warmup=10)
    print(f"trajectory counter={counter}, {n} keyframes, {len(pairs)} records, depth 1-4: "
          f"max abs difference to the recursion {err:.1e}", flush=True)
    print(f"  frontend.trajectory (2 + 12 launches):             median {t_new:8.3f} ms"
          f"   min {m_new:8.3f} ms", flush=True)
    print(f"  Python recursion over lietorch.SE3 (reference):    median {t_old:8.3f} ms"
          f"   min {m_old:8.3f} ms", flush=True)
    print(f"  frontend.trajectory replayed from a graph of 10 calls, per call: "
          f"{_graph_ms(new, 10):8.3f} ms", flush=True)


CASES = [("init", 80), ("init", 96), ("trajectory", 4096)]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs=2, metavar=("KIND", "SIZE"), help="run one case in-process")
    a = ap.parse_args()
    if a.case:
        (run_init if a.case[0] == "init" else run_trajectory)(int(a.case[1]))
    else:
        for kind, size in CASES:
            # a fresh child per case: the parent never opens the device
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", kind,
                                str(size)], timeout=STEP_TIMEOUT)
            if r.returncode != 0:
                sys.exit(f"case {kind} {size} ended with status {r.returncode}; stopping")
