"""Regression guard for the gradient kernels' footprint (no GPU needed: hipcc cross-compiles for gfx950, as tests/test_rollout_resources.py
does): no new kernel goes to scratch or spills a vector register, and launches 1 to 3 -- forward, backward deltas, weight partials -- run
on the matrix core's fp64 instruction.  Nothing else about the ISA is checked."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("forward", "backward", "partial", "reduce", "stats", "pack")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_grad_kernels_keep_their_footprint(tmp_path):
    isa = tmp_path / "grad.s"
    env = dict(os.environ, SMALL="grad", KEEP=str(isa))
    out = subprocess.run(["bash", os.path.join(REPO, "tools", "kernel_resources.sh")], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    by = {}
    for blk in re.split(r"Function Name: *", out.stdout)[1:]:
        name = blk.split("\n")[0].strip()
        for k in KERNELS:
            if "cassie_grad_%s_kernel" % k in name:
                by[k] = (name, blk)
    assert sorted(by) == sorted(KERNELS), out.stdout
    val = lambda blk, key: int(re.search(key + r"[^:]*: *(\d+)", blk).group(1))
    for k, (name, blk) in by.items():
        assert val(blk, "ScratchSize") == 0 and val(blk, "VGPRs Spill") == 0, blk
    asm = isa.read_text()
    for k in ("forward", "backward", "partial"):
        start = asm.index(by[k][0] + ":")
        body = [l.split(";")[0].strip() for l in asm[start: asm.index(".Lfunc_end", start)].split("\n")]
        assert sum(l.startswith("v_mfma_f64_16x16x4_f64") for l in body) >= 1, k
