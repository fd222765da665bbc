"""Build the gfx950 HIP extension in-tree.

Invokes hipcc directly (no hipify, no CUDA shims): the kernel sources in
coda_amd/ops/hip/ are native HIP/CDNA4 code. The resulting
coda_amd/ops/_coda_hip.so is imported by coda_amd.ops and travels with the
repo snapshot to GPU machines (it is git-ignored but not gpurun-ignored).

Usage: python build_hip.py [--force]
"""
from __future__ import annotations

import os
import subprocess
import sys
import sysconfig

REPO = os.path.dirname(os.path.abspath(__file__))
HIP_DIR = os.path.join(REPO, "coda_amd", "ops", "hip")
SRC = [os.path.join(HIP_DIR, f) for f in (
    "module.hip", "pbest.hip", "table.hip", "label.hip", "pair.hip",
    "ingest.hip", "ingest_f16.hip", "ingest_logits.hip", "modelpicker.hip")]
# headers the sources include: part of the up-to-date check only
HDR = [os.path.join(HIP_DIR, f) for f in (
    "wave.h", "beta_grid.h", "host_util.h", "ingest_kernel.h")]
OUT = os.path.join(REPO, "coda_amd", "ops",
                   "_coda_hip.cpython-310-x86_64-linux-gnu.so")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def build(force: bool = False, verbose: bool = True) -> str:
    import torch
    import torch.utils.cpp_extension as ce

    if not force and os.path.exists(OUT):
        newest_src = max(os.path.getmtime(s) for s in SRC + HDR + [__file__])
        if os.path.getmtime(OUT) >= newest_src:
            if verbose:
                print(f"[build_hip] build_mode=reuse (up to date): {OUT}")
            return OUT
    if verbose:
        print("[build_hip] build_mode=compile")

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    includes = ce.include_paths() + [sysconfig.get_paths()["include"]]
    libdirs = ce.library_paths()
    abi = int(torch.compiled_with_cxx11_abi())

    # No tuning flags: the DPP wave scan (wave.h) and the 4-waves/SIMD
    # launch bound (beta_grid.h) that the MI355X sweep chose are written
    # into the sources (sweep record: profiles/README.md). One hipcc call;
    # the sources find their headers next to themselves.
    cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17",
           "-fPIC", "-shared", *SRC, "-o", OUT,
           "-DTORCH_EXTENSION_NAME=_coda_hip",
           "-DTORCH_API_INCLUDE_EXTENSION_H",
           f"-D_GLIBCXX_USE_CXX11_ABI={abi}",
           "-DUSE_ROCM=1", "-D__HIP_PLATFORM_AMD__=1",
           "-fno-gpu-rdc", "-Wno-deprecated-declarations"]
    cmd += [f"-I{p}" for p in includes]
    cmd += [f"-L{p}" for p in libdirs]
    cmd += ["-ltorch", "-ltorch_cpu", "-ltorch_hip", "-lc10", "-lc10_hip",
            "-ltorch_python", "-lamdhip64"]
    if verbose:
        print("[build_hip]", " ".join(cmd))
    subprocess.run(cmd, check=True)
    if verbose:
        print(f"[build_hip] built {OUT}")
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
