"""Timing of the loop-closure back end on the device.

Default mode: cuda_ba.solve_system (Sim3 pose graph, ba.cpp:120-180), median
of HIP-event timings of the whole call (host plan, block assembly, segment
sweeps, border Cholesky).  Graphs (tests/test_pgo.py generators): "loop graph"
= odometry chain + n/50 long loop edges (the shape loop closure builds);
"random 3n edges" = chain + 2n random edges (nearly every pose on the border:
the dense worst case).

--lm: the pose-graph optimiser of dpvo_amd/loop_closure.py on the synthetic
loop of tests/test_pgo_loop_gpu.py (n = 1000 poses, 20 loop edges, f32):
one cuda_ba.pgo_residual(jacobian=True) call, one whole LM iteration, and
the same residual + Jacobians obtained the reference's way on this build: the
Sim3 autograd ops composed as (C * exp(gi) * exp(gj).inv()).log() with seven
backward passes (optim_utils.py:152-161).  Medians of wall-clock timings
around a device synchronisation (the LM iteration syncs by itself)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dpvo_amd  # noqa: E402

cb = dpvo_amd.load_extension("cuda_ba")
dev = torch.device("cuda:0")


def bench_solve():
    from test_pgo import make_loop_graph, make_pgo

    cases = [("loop graph", n, make_loop_graph(n, n // 50, seed=0)) for n in (100, 500, 1000, 2000, 4000)]
    cases += [("random 3n edges", n, make_pgo(n, 3 * n, seed=0)) for n in (100, 500, 1000, 2000)]
    for kind, n, g in cases:
        r = len(g[2])
        Ji, Jj, ii, jj, res = [torch.from_numpy(a).to(dev) for a in g]
        for _ in range(3):
            cb.solve_system(Ji, Jj, ii, jj, res, 1e-4, 1e-4, n - 1)
        ts = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            cb.solve_system(Ji, Jj, ii, jj, res, 1e-4, 1e-4, n - 1)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        print(f"solve_system {kind:16s} n={n} r={r}: {sorted(ts)[5]:.3f} ms", flush=True)


def _median_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    return sorted(ts)[len(ts) // 2]


def bench_lm(n=1000, loops=20):
    from test_pgo_loop_gpu import make_loop

    from dpvo_amd import loop_closure as lc
    from dpvo_amd.lietorch import Sim3

    poses, dS, ii, jj = [t.to(dev) for t in make_loop(n, loops)]
    poses, dS = poses.float(), dS.float()
    Ginv = lc.SE3_to_Sim3(poses).inv().log()
    constants, iii, jjj = lc._edges(n, lc._chain_constants(poses), dS, ii, jj)
    r = len(iii)

    def fused():
        return cb.pgo_residual(Ginv, constants, iii, jjj, True)

    def lm_iteration():
        return lc._lm_iteration(Ginv, constants, iii, jjj, 0.0, 1e-6, -1)

    def composed():
        gi = Ginv[iii].clone().requires_grad_(True)
        gj = Ginv[jjj].clone().requires_grad_(True)
        res = (Sim3(constants) * Sim3.exp(gi) * Sim3.exp(gj).inv()).log()
        rows = [torch.autograd.grad(res[:, k].sum(), (gi, gj), retain_graph=True) for k in range(7)]
        return res, torch.stack([a for a, _ in rows], 1), torch.stack([b for _, b in rows], 1)

    res, Ji, Jj = fused()
    cres, cJi, cJj = composed()
    print(f"n={n} loops={loops} r={r} f32; fused vs composed max abs diff: res "
          f"{(res - cres).abs().max().item():.2e} J_i {(Ji - cJi).abs().max().item():.2e} "
          f"J_j {(Jj - cJj).abs().max().item():.2e}", flush=True)
    print(f"pgo_residual(jacobian=True): {_median_ms(fused):.3f} ms", flush=True)
    print(f"one LM iteration:            {_median_ms(lm_iteration):.3f} ms", flush=True)
    print(f"composed autograd ops:       {_median_ms(composed):.3f} ms", flush=True)
    print(f"(solve_system alone:         {_median_ms(lambda: cb.solve_system(Ji, Jj, iii, jjj, res, 0.0, 1e-6, -1)):.3f} ms)",
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lm", action="store_true", help="time the pose-graph optimiser instead")
    a = ap.parse_args()
    bench_lm() if a.lm else bench_solve()
