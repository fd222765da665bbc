"""Resource audit of the logits ingest kernels (no GPU needed: hipcc
cross-compiles gfx950). ingest_logits.hip holds 3 logit wire dtypes x 4
storage dtypes x {vector, scalar} instantiations of one kernel. The
launch geometry plans for two 512-thread blocks per CU (80 KB of LDS
each), which is 4 waves per SIMD: every instantiation must compile
without scratch and within 128 VGPRs, at an occupancy of at least 4."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC),
                                reason="hipcc not available")


def test_ingest_logits_kernels_resource_envelope(tmp_path):
    import sysconfig
    import torch
    import torch.utils.cpp_extension as ce
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
           "-c", os.path.join(REPO, "coda_amd", "ops", "hip",
                              "ingest_logits.hip"),
           "-o", str(tmp_path / "ingest_logits.o"),
           "-Rpass-analysis=kernel-resource-usage",
           "-DTORCH_EXTENSION_NAME=_kra", "-DTORCH_API_INCLUDE_EXTENSION_H",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch.compiled_with_cxx11_abi())}",
           "-DUSE_ROCM=1", "-D__HIP_PLATFORM_AMD__=1"]
    cmd += [f"-I{p}" for p in ce.include_paths()]
    cmd += [f"-I{sysconfig.get_paths()['include']}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name:\s*(\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
        for key, pat in (("vgpr", r" VGPRs:\s*(\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]:\s*(\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]:\s*(\d+)")):
            m = re.search(pat, line)
            if m and cur:
                kernels[cur][key] = int(m.group(1))
    ingest = {k: v for k, v in kernels.items() if "ingest_logits_kernel" in k}
    # 3 wire dtypes x 4 storage dtypes x {vector, scalar}
    assert len(ingest) == 24, sorted(ingest)
    for name, info in ingest.items():
        assert info["scratch"] == 0, (name, info)
        assert info["vgpr"] <= 128, (name, info)
        assert info["occupancy"] >= 4, (name, info)
