"""Resource audit of the hit-sparse ModelPicker kernel (no GPU needed:
hipcc cross-compiles gfx950). modelpicker.hip instantiates the kernel for
1..16 sorted positions per lane, each with a scalar row load and - where
the count is even - a vector one. Every instantiation keeps its row,
the staged (p, q) pairs and the prefetched next row in registers: it must
compile without scratch, within 128 VGPRs, at 4 waves/SIMD or better."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC),
                                reason="hipcc not available")


def test_modelpicker_kernels_resource_envelope(tmp_path):
    import sysconfig
    import torch
    import torch.utils.cpp_extension as ce
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
           "-c", os.path.join(REPO, "coda_amd", "ops", "hip",
                              "modelpicker.hip"),
           "-o", str(tmp_path / "modelpicker.o"),
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
    mp = {k: v for k, v in kernels.items() if "modelpicker_dev_kernel" in k}
    # 16 position counts x scalar loads + 8 even counts x vector loads
    assert len(mp) == 24, sorted(mp)
    for name, info in mp.items():
        assert info["scratch"] == 0, (name, info)
        assert info["vgpr"] <= 128, (name, info)
        assert info["occupancy"] >= 4, (name, info)
