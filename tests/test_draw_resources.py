"""Regression guard for the draw kernels' footprint (no GPU needed: hipcc cross-compiles for gfx950, as tests/test_norm_resources.py
does): the two kernels are found, neither goes to scratch or spills a vector register.  Nothing else about the ISA is checked."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("cassie_draw_kernel", "cassie_draw_perm_kernel")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_draw_kernels_keep_their_footprint():
    env = dict(os.environ, SMALL="draw")
    out = subprocess.run(["bash", os.path.join(REPO, "tools", "kernel_resources.sh")], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    by = {}
    for blk in re.split(r"Function Name: *", out.stdout)[1:]:
        name = blk.split("\n")[0].strip()
        for k in KERNELS:
            if re.search(r"%s(?![a-z_])" % k, name):
                by[k] = (name, blk)
    assert sorted(by) == sorted(KERNELS), out.stdout
    val = lambda blk, key: int(re.search(key + r"[^:]*: *(\d+)", blk).group(1))
    for k, (name, blk) in by.items():
        assert val(blk, "ScratchSize") == 0 and val(blk, "VGPRs Spill") == 0, blk
