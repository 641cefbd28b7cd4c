"""Regression guard for the normaliser kernels' footprint (no GPU needed: hipcc cross-compiles for gfx950, as tests/test_opt_resources.py
does): the five kernels are found, none goes to scratch or spills a vector register.  Nothing else about the ISA is checked."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("sum", "mean", "sq", "merge", "write")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_norm_kernels_keep_their_footprint():
    env = dict(os.environ, SMALL="norm")
    out = subprocess.run(["bash", os.path.join(REPO, "tools", "kernel_resources.sh")], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    by = {}
    for blk in re.split(r"Function Name: *", out.stdout)[1:]:
        name = blk.split("\n")[0].strip()
        for k in KERNELS:
            if "cassie_norm_%s_kernel" % k in name:
                by[k] = (name, blk)
    assert sorted(by) == sorted(KERNELS), out.stdout
    val = lambda blk, key: int(re.search(key + r"[^:]*: *(\d+)", blk).group(1))
    for k, (name, blk) in by.items():
        assert val(blk, "ScratchSize") == 0 and val(blk, "VGPRs Spill") == 0, blk
