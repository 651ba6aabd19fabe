"""In-tree build of the MI355X (gfx950) native code.

    python -m dpvo_amd.build            # build everything (incremental)
    python -m dpvo_amd.build --force    # rebuild

Products (dpvo_amd/_native/, git-ignored, shipped to the GPU box by gpurun):
  libdpvo_hot.so                      HIP kernels + the C ABI of include/dpvo_hot.h
  cuda_corr.<ext>, cuda_ba.<ext>,     pybind11 extension modules with the
  lietorch_backends.<ext>             reference's module / function names,
                                      thin wrappers over libdpvo_hot.so
  dpvo_update.<ext>                   the update operator (PyTorch in the reference)
  dpvo_encoder.<ext>                  the feature encoders (PyTorch in the reference)

hipcc compiles the kernels directly for gfx950; the extension modules are
host-only C++ compiled with g++ against the PyTorch-ROCm headers (no hipify,
no JIT cache outside the tree).  Every source, HIP or C++, becomes one object
under _native/obj/, rebuilt only when it or a header it includes is newer; all
stale objects compile concurrently in one pool (MAX_JOBS, at most 16), then
the library and the five modules are linked, the modules side by side.
"""
from __future__ import annotations

import argparse
import os
import shlex
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "_native")
INCLUDE = os.path.join(REPO, "include")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("DPVO_OFFLOAD_ARCH", "gfx950")

HIP_SOURCES = ["corr.hip", "corr_nhwc.hip", "corr_nchw.hip", "ba.hip", "ba_window.hip", "ba_large.hip", "lie.hip", "pgo.hip", "pg.hip",
               "keyframe.hip", "spd_solve.hip", "ransac.hip", "update_op.hip", "update_bwd.hip", "encoder.hip", "encoder_bwd.hip",
               "frontend.hip", "ba_layer.hip", "tracker.hip", "match.hip", "triangulate.hip", "train.hip", "stream.hip", "evaluate.hip", "dataset.hip"]
# module -> its sources; cuda_ba is one module split by subsystem
EXTENSIONS = {
    "cuda_corr": ["ext_cuda_corr.cpp"],
    "cuda_ba": ["ext_cuda_ba.cpp", "ext_ba_solve.cpp", "ext_ba_graph.cpp", "ext_ba_train.cpp",
                "ext_ba_tracker.cpp"],
    "lietorch_backends": ["ext_lietorch.cpp"],
    "dpvo_update": ["ext_update.cpp"],
    "dpvo_encoder": ["ext_encoder.cpp"],
}
EXT_HEADERS = ["ext_common.hpp"]  # what the ext_*.cpp include besides dpvo_hot.h
HEADERS = ["common.hpp", "ba_device.hpp", "ba_solve.hpp", "pyr_insert.hpp", "ba_bgj.hpp",
           "sim3.hpp", "lie_se3.hpp", "ba_paths.hpp", "corr_paths.hpp", "encoder_layout.hpp", "update_layout.hpp", "umeyama.hpp", "radix_select.hpp"]
# per-source device flags.  The BA window kernel is a chain of short dependent
# steps run by few waves: clang's SLP vectoriser packs its scalar fp32 math into
# v_pk_fma_f32 and pays for it with register-pair v_mov shuffles (3x the
# instructions of the 6x6 pivot factorisation), so it is off there.
SOURCE_FLAGS = {"ba_window.hip": ["-fno-slp-vectorize"]}


def _git_rev():
    try:
        return subprocess.check_output(["git", "-C", REPO, "rev-parse", "--short", "HEAD"],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "nogit"


def _run(cmd, verbose):
    if verbose:
        print("+", " ".join(shlex.quote(c) for c in cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout.decode(errors="replace"))
        raise RuntimeError(f"build step failed: {cmd[0]} -> {cmd[-1]}")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def lib_path():
    return os.path.join(OUT, "libdpvo_hot.so")


def ext_suffix():
    return sysconfig.get_config_var("EXT_SUFFIX")


def build(force=False, verbose=False):
    os.makedirs(OUT, exist_ok=True)
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    api = os.path.join(INCLUDE, "dpvo_hot.h")
    hdr = [api] + [os.path.join(CSRC, h) for h in HEADERS]
    ext_hdr = [api] + [os.path.join(CSRC, h) for h in EXT_HEADERS]
    lib = lib_path()
    objdir = os.path.join(OUT, "obj")
    os.makedirs(objdir, exist_ok=True)

    import torch
    from torch.utils import cpp_extension as ce

    tinc = ce.include_paths()
    tlib = ce.library_paths()[0]
    abi = []
    for getter in ("_get_pybind11_abi_build_flags", "_get_glibcxx_abi_build_flags"):
        fn = getattr(ce, getter, None)
        if fn is not None:
            abi += list(fn())
    pyinc = sysconfig.get_paths()["include"]
    del torch

    def obj_of(src):
        return os.path.join(objdir, os.path.splitext(src)[0] + ".o")

    # one object per source (incremental).  The extension sources go first:
    # each is one long single-threaded g++ run over the PyTorch headers.
    cmds = []
    for name, sources in EXTENSIONS.items():
        for src in sources:
            srcp = os.path.join(CSRC, src)
            if force or _stale(obj_of(src), [srcp] + ext_hdr + [__file__]):
                cmds.append(["g++", "-O2", "-std=c++17", "-fPIC", "-c", "-fvisibility=hidden",
                             "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
                             "-DTORCH_API_INCLUDE_EXTENSION_H", f"-DTORCH_EXTENSION_NAME={name}",
                             *abi, f"-I{INCLUDE}", f"-I{CSRC}", *[f"-I{p}" for p in tinc],
                             f"-I{ROCM}/include", f"-I{pyinc}", srcp, "-o", obj_of(src)])
    for src in HIP_SOURCES:
        srcp = os.path.join(CSRC, src)
        if force or _stale(obj_of(src), [srcp] + hdr + [__file__]):
            cmds.append([hipcc, "-O3", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-c",
                         "-fvisibility=hidden", "-mcode-object-version=5", "-Wno-unused-result",
                         f"-I{INCLUDE}", f'-DDPVO_GIT_REV="{_git_rev()}"',
                         *SOURCE_FLAGS.get(src, []), srcp, "-o", obj_of(src)])
    # the objects are independent: compile them concurrently (bounded by the
    # host's share of CPUs; MAX_JOBS is honoured as on the GPU box)
    jobs = max(1, min(int(os.environ.get("MAX_JOBS", os.cpu_count() or 1)), 16))
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(lambda c: _run(c, verbose), cmds))
        hip_objs = [obj_of(s) for s in HIP_SOURCES]
        if force or _stale(lib, hip_objs):
            _run([hipcc, f"--offload-arch={ARCH}", "-fPIC", "-shared", *hip_objs, "-o", lib], verbose)
        links = []
        for name, sources in EXTENSIONS.items():
            target = os.path.join(OUT, name + ext_suffix())
            objs = [obj_of(s) for s in sources]
            if force or _stale(target, objs + [lib]):
                links.append(["g++", "-shared", *objs, "-o", target, f"-L{OUT}", "-ldpvo_hot",
                              f"-L{tlib}", "-lc10", "-lc10_hip", "-ltorch", "-ltorch_cpu",
                              "-ltorch_hip", "-ltorch_python", "-Wl,-rpath,$ORIGIN",
                              f"-Wl,-rpath,{tlib}"])
        list(ex.map(lambda c: _run(c, verbose), links))
    return OUT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("-v", "--verbose", action="store_true")
    a = ap.parse_args()
    out = build(force=a.force, verbose=a.verbose)
    print("built", out)


if __name__ == "__main__":
    main()
