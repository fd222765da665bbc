"""Compare the gfx950 device code of two HIP source directories.

Every .hip file of each directory is compiled device-only to assembly;
each function's text is keyed by its mangled name, with local-label
numbers normalised and comment lines dropped, and compared across the two
trees together with the kernel-resource-usage remarks (SGPR, VGPR, AGPR,
scratch, LDS, occupancy). Exit status 0 means: same set of names,
identical text and identical resources for every one of them.

Usage:
  python scripts/kernel_isa_diff.py DIR_A DIR_B [--defs-a="-DX=1 ..."]
                                                [--defs-b="..."] [--jobs N]

--defs-a/--defs-b carry the -D flags that the tree's own build_hip.py
passes beyond the common ones (none for this tree).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import difflib
import glob
import os
import re
import subprocess
import sys
import sysconfig
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
RES = (("sgpr", r"SGPRs:\s*(\d+)"), ("vgpr", r"VGPRs:\s*(\d+)"),
       ("agpr", r"AGPRs:\s*(\d+)"),
       ("scratch", r"ScratchSize \[bytes/lane\]:\s*(\d+)"),
       ("lds", r"LDS Size \[bytes/block\]:\s*(\d+)"),
       ("occupancy", r"Occupancy \[waves/SIMD\]:\s*(\d+)"))


def common_flags():
    import torch
    import torch.utils.cpp_extension as ce
    abi = int(torch.compiled_with_cxx11_abi())
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17",
             "--cuda-device-only", "-S", "-fno-gpu-rdc",
             "-Rpass-analysis=kernel-resource-usage",
             "-DTORCH_EXTENSION_NAME=_coda_hip",
             "-DTORCH_API_INCLUDE_EXTENSION_H",
             f"-D_GLIBCXX_USE_CXX11_ABI={abi}",
             "-DUSE_ROCM=1", "-D__HIP_PLATFORM_AMD__=1",
             "-Wno-deprecated-declarations"]
    flags += [f"-I{p}" for p in ce.include_paths()]
    flags += [f"-I{sysconfig.get_paths()['include']}"]
    return flags


def compile_one(src, flags, tmp):
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    r = subprocess.run([HIPCC, *flags, f"-I{os.path.dirname(src)}", src,
                        "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{src}:\n{r.stderr[-3000:]}")
    with open(out) as f:
        return f.read(), r.stderr


def parse_asm(text):
    """{mangled name: normalised lines} for every function; kernel names."""
    funcs, kernels, cur = {}, set(), None
    for line in text.splitlines():
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernels.add(m.group(1))
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            cur = None
            continue
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        funcs[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return funcs, kernels


def parse_remarks(stderr):
    res, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name:\s*(\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
        for key, pat in RES:
            m = re.search(pat, line)
            if m and cur:
                res[cur][key] = int(m.group(1))
    return res


def scan(directory, defs, jobs):
    flags = common_flags() + defs
    srcs = sorted(glob.glob(os.path.join(directory, "*.hip")))
    funcs, kernels, res, where = {}, set(), {}, {}
    with tempfile.TemporaryDirectory() as tmp, \
            cf.ThreadPoolExecutor(jobs) as pool:
        for src, (asm, err) in zip(
                srcs, pool.map(lambda s: compile_one(s, flags, tmp), srcs)):
            f, k = parse_asm(asm)
            for name in f:
                if name in funcs:
                    raise RuntimeError(f"{name} emitted by two sources")
                where[name] = os.path.basename(src)
            funcs.update(f)
            kernels |= k
            res.update(parse_remarks(err))
    return funcs, kernels, res, where


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--defs-a", default="")
    ap.add_argument("--defs-b", default="")
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    fa, ka, ra, wa = scan(a.dir_a, a.defs_a.split(), a.jobs)
    fb, kb, rb, wb = scan(a.dir_b, a.defs_b.split(), a.jobs)

    bad = 0
    for name in sorted(set(fa) ^ set(fb)):
        print(f"ONLY IN {'A' if name in fa else 'B'}: {name}")
        bad += 1
    print(f"{'function':<70} {'A':<18} {'B':<18} lines  text  resources")
    for name in sorted(set(fa) & set(fb)):
        same_text = fa[name] == fb[name]
        same_res = ra.get(name) == rb.get(name)
        ndiff = 0
        if not same_text:
            ndiff = sum(1 for d in difflib.unified_diff(
                fa[name], fb[name], lineterm="", n=0)
                if d[:1] in "+-" and d[:3] not in ("+++", "---"))
        bad += (not same_text) + (not same_res)
        tag = "" if name in ka else " (device fn)"
        print(f"{name + tag:<70} {wa[name]:<18} {wb[name]:<18} "
              f"{len(fa[name]):>5}  "
              f"{'same' if same_text else f'DIFF({ndiff})'}  "
              f"{'same' if same_res else f'{ra.get(name)} != {rb.get(name)}'}")
    print(f"kernels: A={len(ka)} B={len(kb)} names_equal={ka == kb}; "
          f"functions compared={len(set(fa) & set(fb))}; mismatches={bad}")
    return 1 if bad or ka != kb else 0


if __name__ == "__main__":
    sys.exit(main())
