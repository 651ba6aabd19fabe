"""Timing of the loop-closure measurement: loop_closure.ransac_umeyama on the
device against the numpy restatement on the host, on the same inputs.

Cases: tests/umeyama_restatement.make_case with N = 512 and 2048 matched
points, 60 % outliers, H = 400 hypotheses (what close_loop asks for).  The
default early_exit = 100 ends the reference's loop after a few hypotheses;
early_exit = N makes it look at all 400.  The device scores all H hypotheses
either way (one wave each), so its time does not depend on early_exit.

Device: median of HIP-event timings around the whole Python call with given
samples (two kernels plus the small tensor ops around them), then of the call
that also draws its samples (rand + argsort of [H, N]).  Host: median wall
clock of umeyama_restatement.ransac_umeyama (numpy, one hypothesis after the
other, stopping at the early exit as the reference does).  The reference runs
the same loop under numba, which is not installed here: the numpy figure is an
upper bound for it, not its time.  The reference also copies both clouds to
the host first; that copy is not timed.

Each case runs in a child process under a time limit of its own, so a hang
ends the script instead of holding the device.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(512, 400), (2048, 400)]
STEP_TIMEOUT = 120  # seconds per case


def run_case(N, H):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import umeyama_restatement as U

    from dpvo_amd import loop_closure as lc

    dev = torch.device("cuda:0")
    src, dst, samples = U.make_case(N, H, 10, 0.6)
    ds, dd, dsmp = [torch.from_numpy(a).to(dev) for a in (src, dst, samples)]
    dsmp = dsmp.int()

    def device_ms(fn, reps=50, warmup=5):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    full = U.ransac_umeyama(src, dst, samples, early_exit=N)
    stops = {100: U.ransac_umeyama(src, dst, samples)["stop"], N: full["stop"]}

    def host_ms(early_exit, reps=5):
        # the restatement scores every hypothesis it is given (for counts[]);
        # the reference's loop ends at the stop index, so it gets that many
        upto = samples[:stops[early_exit] + 1]
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            U.ransac_umeyama(src, dst, upto, early_exit=early_exit)
            ts.append(1e3 * (time.perf_counter() - t))
        return sorted(ts)[len(ts) // 2]

    cb = lc.cuda_ba
    est = lc.ransac_umeyama(ds, dd, samples=dsmp, early_exit=N)
    assert est.info.tolist() == [full["num_inliers"], full["winner"], full["stop"], 0]
    err = max(np.abs(est.R.cpu().numpy() - full["R"]).max(),
              np.abs(est.t.cpu().numpy() - full["t"]).max(), abs(float(est.s) - full["s"]))
    print(f"N={N} H={H} f64: {full['num_inliers']} inliers, device against numpy max abs "
          f"error of R / t / s {err:.1e}", flush=True)
    t_kernels = device_ms(lambda: cb.ransac_umeyama(ds, dd, dsmp, 0.1, 100, check_samples=False))
    t_drawn = device_ms(lambda: lc.ransac_umeyama(ds, dd, iterations=H))
    print(f"  device, given samples (score + select):  {t_kernels:8.3f} ms", flush=True)
    print(f"  device, samples drawn in the call:       {t_drawn:8.3f} ms", flush=True)
    for ee in (100, N):
        print(f"  numpy on the host, early_exit={ee:<5d} ({stops[ee] + 1:3d} hypotheses): "
              f"{host_ms(ee):8.3f} ms", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, nargs=2, metavar=("N", "H"), help="run one case in-process")
    a = ap.parse_args()
    if a.case:
        run_case(*a.case)
    else:
        for N, H in CASES:
            # a fresh child per case: the parent never opens the device
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(N), str(H)],
                               timeout=STEP_TIMEOUT)
            if r.returncode != 0:
                sys.exit(f"case N={N} H={H} ended with status {r.returncode}; stopping")
