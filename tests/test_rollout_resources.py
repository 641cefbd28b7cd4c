"""Regression guard for the rollout kernels' footprint (no GPU needed: hipcc cross-compiles for gfx950, as tests/test_kernel_resources.py
does for the step kernel): nothing goes to scratch, no vector register is spilled, and no kernel takes LDS -- csrc/rollout_kernels.h
declares none (an array of a four-word struct once went there by the compiler's own choice: 4 KiB a workgroup of the record kernel)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("cassie_rollout_record_kernel", "cassie_rollout_finish_kernel", "cassie_rollout_reduce_kernel", "cassie_rollout_square_kernel",
           "cassie_rollout_scale_kernel")
DECLARED_LDS = 0       # bytes of WV_SHARED in csrc/rollout_kernels.h


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_rollout_kernels_keep_their_footprint():
    with open(os.path.join(REPO, "cassie-mujoco-sim_amd", "csrc", "rollout_kernels.h")) as f:
        assert "WV_SHARED" not in f.read()            # (what DECLARED_LDS says)
    out = subprocess.run(["bash", os.path.join(REPO, "tools", "kernel_resources.sh")], env=dict(os.environ, SMALL="rollout"),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    by = {}
    for blk in re.split(r"Function Name: *", out.stdout)[1:]:
        name = blk.split("\n")[0].strip()
        for k in KERNELS:
            if k in name:
                by[k] = blk
    assert sorted(by) == sorted(KERNELS), out.stdout
    val = lambda blk, key: int(re.search(key + r"[^:]*: *(\d+)", blk).group(1))
    for k, blk in by.items():
        assert val(blk, "ScratchSize") == 0 and val(blk, "VGPRs Spill") == 0, blk
        assert val(blk, "LDS Size") <= DECLARED_LDS, blk
