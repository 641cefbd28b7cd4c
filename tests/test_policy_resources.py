"""Regression guard for the policy kernels' footprint (no GPU needed: hipcc cross-compiles for gfx950, as tests/test_kernel_resources.py
does for the step kernel): the layers run on the matrix core's fp64 instruction, nothing goes to scratch, and the two activation
buffers -- dynamic LDS the launcher sizes by the policy's widths, at most 64 KiB (tests/test_policy.py) -- are all the LDS a workgroup
takes: the kernel has no static LDS beside them."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_policy_kernels_keep_their_footprint(tmp_path):
    isa = tmp_path / "policy.s"
    env = dict(os.environ, SMALL="policy", KEEP=str(isa))
    out = subprocess.run(["bash", os.path.join(REPO, "tools", "kernel_resources.sh")], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    blocks = re.split(r"Function Name: *", out.stdout)[1:]
    by = {}
    for blk in blocks:
        name = blk.split("\n")[0].strip()
        by["pack" if "policy_pack_kernel" in name else "policy" if "cassie_policy_kernel" in name else name] = blk
    assert "policy" in by and "pack" in by, out.stdout
    val = lambda blk, key: int(re.search(key + r"[^:]*: *(\d+)", blk).group(1))
    assert val(by["policy"], "ScratchSize") == 0 and val(by["policy"], "VGPRs Spill") == 0, by["policy"]
    assert val(by["policy"], "LDS Size") <= 65536, by["policy"]
    assert val(by["pack"], "ScratchSize") == 0 and val(by["pack"], "LDS Size") == 0, by["pack"]
    # the instructions of the policy kernel alone: from its label to its end
    asm = isa.read_text()
    start = asm.index("_ZN2ck20cassie_policy_kernelENS_8PolicyIOE:")
    body = [l.split(";")[0].strip() for l in asm[start: asm.index(".Lfunc_end", start)].split("\n")]
    assert sum(l.startswith("v_mfma_f64_16x16x4_f64") for l in body) >= 1
    assert not any(l.startswith(("scratch_load", "scratch_store")) for l in body)
