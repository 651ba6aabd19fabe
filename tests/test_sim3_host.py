"""CPU: dpvo_amd/csrc/sim3.hpp compiled for the host (tests/sim3_host_main.cpp,
built by the hipcc of dpvo_amd/build.py; no HIP call, no device) over the fp64
(theta, sigma) sweep of tests/sim3_bands.py, all 11 forward and 8 backward ops
of lietorch group 4, against tests/sim3_restatement.py.  This is the CPU unit
test the header speaks of: its branches (series / recurrence / closed form of
w_coeffs, atan series / atan2 / w < 0 of logm) and their Dual derivatives with
the host compiler and libm; test_sim3_bands_gpu.py runs the same rows through
the kernels.  A missing compiler is a failure, not a skip.

Bound 1e-12 in the row measure |got - ref| / max(1, max |ref| of the row):
about 20 times the largest error measured (5.5e-14) to allow for other libm
versions.  Measured maxima on an x86-64 host (sweep / block case):
  forward   exp 4.4e-15 / 1.8e-15   log 1.5e-15 / 1.9e-15   inv 1.3e-15 / 4.1e-16
            mul 9.5e-16 / 8.4e-16   adj 1.3e-15 / 5.9e-16   adjT 7.8e-16 / 4.5e-16
            act 6.7e-16 / 5.1e-16   act4 8.7e-16 / 5.0e-16  matrix 0 / 0
            projector 0 / 0         Jinv 5.5e-14 / 3.6e-15
  backward  exp 4.9e-14 / 3.0e-15   log 5.2e-14 / 2.7e-15   inv 1.3e-15 / 8.9e-16
            mul 1.7e-14 / 2.4e-15   adj 1.2e-15 / 1.2e-15   adjT 1.2e-15 / 1.7e-15
            act 7.1e-16 / 5.5e-16   act4 9.7e-16 / 5.2e-16
(matrix and projector are 0 because the reference forms the same products.)
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import sim3_bands as B
from dpvo_amd import build as native_build

BOUND = 1e-12
QNORM_BOUND = 1e-14  # a normalised fp64 quaternion: a few roundoffs
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The stand-alone program, compiled once."""
    exe = str(tmp_path_factory.mktemp("sim3_host") / "sim3_host")
    hipcc = os.path.join(native_build.ROCM, "bin", "hipcc")
    assert os.path.exists(hipcc), f"{hipcc}: the compiler of dpvo_amd/build.py is missing"
    cmd = [hipcc, "-x", "hip", f"--offload-arch={native_build.ARCH}", "-O3", "-std=c++17",
           f"-I{native_build.CSRC}", f"-I{native_build.INCLUDE}",
           os.path.join(HERE, "sim3_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def _run(host, tmp_path, direction, op, blocks, widths):
    """blocks: fp64 tensors [n, w] written one after the other; returns the
    output blocks of the given widths."""
    n = len(blocks[0])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for b in blocks:
            f.write(np.ascontiguousarray(b.numpy(), dtype=np.float64).tobytes())
    r = subprocess.run([host, direction, str(B.OP_INDEX[op]), str(n), fin, fout],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, (r.returncode, r.stdout.decode(errors="replace"))
    flat = np.fromfile(fout, dtype=np.float64)
    assert flat.size == n * sum(widths)
    outs, at = [], 0
    for w in widths:
        outs.append(torch.from_numpy(flat[at:at + n * w].reshape(n, w).copy()))
        at += n * w
    return outs


FWD_OUT = {"exp": 8, "log": 7, "inv": 8, "mul": 8, "adj": 7, "adjT": 7, "act": 3, "act4": 4,
           "matrix": 16, "projector": 64, "Jinv": 7}
BWD_OUT = {"exp": (7,), "log": (8,), "inv": (8,), "mul": (8, 8), "adj": (8, 7), "adjT": (8, 7),
           "act": (8, 3), "act4": (8, 4)}


@pytest.mark.parametrize("case", ["sweep", "block"])
@pytest.mark.parametrize("op", B.FWD_OPS)
def test_header_forward_on_the_host(host, tmp_path, op, case):
    x, y, _, ref = B.case(op, False, "f64", case)
    out, = _run(host, tmp_path, "fwd", op, [t for t in (x, y) if t is not None], [FWD_OUT[op]])
    err, qerr = B.forward_error(op, out, ref)
    print(f"SIM3 HOST fwd op={op} {case} err={err:.3e} qnorm={qerr:.1e}")
    assert err <= BOUND
    assert qerr <= QNORM_BOUND


@pytest.mark.parametrize("case", ["sweep", "block"])
@pytest.mark.parametrize("op", B.BWD_OPS)
def test_header_backward_on_the_host(host, tmp_path, op, case):
    x, y, g, refs = B.case(op, True, "f64", case)
    outs = _run(host, tmp_path, "bwd", op, [t for t in (g, x, y) if t is not None], BWD_OUT[op])
    err = B.backward_error(outs, refs)
    print(f"SIM3 HOST bwd op={op} {case} err={err:.3e}")
    assert err <= BOUND
