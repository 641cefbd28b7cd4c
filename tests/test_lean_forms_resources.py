"""What leaving the read-out code, the forward-mode exits and the stage stamps out of the fast kernels buys, as the compiler counts it (no
GPU needed: hipcc cross-compiles): the lean two-wave fast kernel of cassie.xml -- the kernel the benchmark spends its time in --
against the figures of the same kernel before the two feature bits existed (profiles/round7/lean_forms_resources.txt, the column
"parent": commit 1c63e97, same flags).  The bounds below ARE that column: the lean kernel must never again cost more than the kernel
that carried everything."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# profiles/round7/lean_forms_resources.txt, column "parent"
PARENT = dict(vgprs=246, sgpr_spills=349, scratch=132, instructions=21719, lines=24885, writelanes=349, readlanes=1285, nops=587, global_stores=227)
COST_MEMTIMES = 2       # io.cost's pair (cassie_step_kernel: t0 and the env's end), counted in the parent: 43 in all, 41 of them stamps


def instructions(asm):
    """The instruction lines of a kernel's ISA: no labels, directives or comments."""
    body = [l.split(";")[0].strip() for l in asm.split("\n")]
    return [l for l in body if l and not l.startswith((".", "//")) and not l.endswith(":") and re.match(r"[a-z_0-9]+(\s|$)", l)]


def figures(remarks, asm):
    val = lambda key: int(re.search(key + r"[^:]*: *(\d+)", remarks).group(1))
    ins = instructions(asm)
    count = lambda prefix: sum(l.startswith(prefix) for l in ins)
    return dict(vgprs=val("VGPRs"), sgpr_spills=val("SGPRs Spill"), vgpr_spills=val("VGPRs Spill"), scratch=val("ScratchSize"), instructions=len(ins),
                lines=asm.count("\n"), memtimes=count("s_memtime"), writelanes=count("v_writelane"), readlanes=count("v_readlane"), nops=count("s_nop"),
                global_stores=count("global_store"))


def kernarg_loads(asm):
    """[(first byte, end byte)] of the scalar loads from the kernel's argument block (its address is in s[0:1] at entry)."""
    out = []
    for l in instructions(asm):
        m = re.match(r"s_load_dword(x(\d+))?\s+\S+,\s*s\[0:1\],\s*(0x[0-9a-f]+|\d+)", l)
        if m:
            off = int(m.group(3), 0)
            out.append((off, off + 4 * int(m.group(2) or 1)))
    return out


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_lean_cassie_two_wave_kernel_has_no_stamp_no_read_out_and_costs_no_more_than_the_parent(tmp_path, built):
    isa = tmp_path / "lean.s"
    env = dict(os.environ, MAXRS="31", NW="2", KEEP=str(isa))
    out = subprocess.run(["bash", os.path.join(REPO, "tools", "kernel_resources.sh")], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FEAT=0," in out.stdout and "SERVE=0>" in out.stdout, out.stdout      # (the lean form: neither FEAT_READOUT nor FEAT_PROF)
    asm = isa.read_text()
    f = figures(out.stdout, asm)
    print(f)
    # no stage stamp: the shader clock is read for io.cost alone
    assert f["memtimes"] == COST_MEMTIMES, f
    # no store through the read-out pointer, no stamp through the profile pointer: the kernel does not even load either from its
    # argument block -- while it does load their neighbours (the positive control: io.cost)
    import emu_py
    off = np.zeros(5, dtype=np.uint64)
    E = emu_py.lib()
    E.emu_physio_offsets.argtypes, E.emu_physio_offsets.restype = [ctypes.c_void_p], None
    E.emu_physio_offsets(off.ctypes.data)
    ext, prof, integrate, cost, size = (int(v) for v in off)
    loads = kernarg_loads(asm)
    covered = lambda at, n: [(a, e) for a, e in loads if a < at + n and at < e]
    assert loads and max(e for _, e in loads) <= size, loads
    assert covered(cost, 8), "the scan of the argument block's loads does not see the load of io.cost"
    assert not covered(ext, 8), ("io.ext is loaded", covered(ext, 8))
    assert not covered(prof, 8), ("io.prof is loaded", covered(prof, 8))
    # ... and the allocator got something back, not less: no figure above the parent's
    for k, bound in PARENT.items():
        assert f[k] <= bound, (k, f[k], bound)
