"""What the accumulation code costs the two-wave fast kernel of cassie.xml, as the compiler counts it (no GPU needed: hipcc
cross-compiles): the FEAT_SUMS sibling (csrc/kernels_cassie_sums.hip) against its lean sibling compiled in the same build, with the same
flags.  The sibling must be placed like the lean form -- two waves per SIMD, four envs per CU -- and may cost what DESIGN.md 4.7
records, measured: no vector spill, the same scratch frame, 3 more spilled scalars (the block's row pointer and the launch's contact-force
flag live across the substep loop)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured in this build: lean 0 / 132 B / 171, sums 0 / 132 B / 174
DELTA = dict(vgpr_spills=0, scratch=0, sgpr_spills=3)


def _figures(**extra):
    env = dict(os.environ, MAXRS="31", NW="2", **extra)
    out = subprocess.run(["bash", os.path.join(REPO, "tools", "kernel_resources.sh")], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    val = lambda key: int(re.search(key + r"[^:]*: *(\d+)", out.stdout).group(1))
    return out.stdout, dict(vgpr_spills=val("VGPRs Spill"), scratch=val("ScratchSize"), sgpr_spills=val("SGPRs Spill"), lds=val("LDS Size"),
                            occupancy=val("Occupancy"))


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_the_accumulating_two_wave_fast_kernel_is_placed_like_the_lean_one():
    text, lean = _figures()
    assert "SERVE=0>" in text, text
    text, sums = _figures(SUMS="1")
    assert "SERVE=16>" in text, text
    print("lean", lean, "sums", sums)
    assert sums["occupancy"] == 2, sums             # two waves per SIMD: 256 registers each
    assert sums["lds"] <= 40960, sums               # four two-wave workgroups per CU
    for k, d in DELTA.items():
        assert sums[k] <= lean[k] + d, (k, sums[k], lean[k], d)
