"""What the static ISA tests share (test_isa.py, test_batch_cpu.py): the device-only hipcc command line, the parser of its
assembly output and the wait-state check behind v_rsq_f32.  A plain helper module; no GPU needed (hipcc cross-compiles)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = "/opt/rocm/bin/hipcc"


def compile_isa(out_dir, source):
    """gfx950 assembly text of nbody_amd/csrc/<source>: the flags of nbody_amd/csrc/Makefile (HIPFLAGS), device side only."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = out_dir / (os.path.splitext(source)[0] + ".s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-Wno-unused-command-line-argument",
           f"-I{ROOT}/include", f"-I{ROOT}/nbody_amd/csrc", "--cuda-device-only", "-S", "-o", str(out),
           os.path.join(ROOT, "nbody_amd", "csrc", source)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out.read_text()


def functions(text):
    """name -> list of instruction lines (labels, directives and comments dropped)."""
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_ZN2nb\S+):", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        if name is None:
            continue
        ins = line.split(";")[0].strip()
        if not ins or ins.startswith(".") or ins.endswith(":"):
            continue
        out[name].append(ins)
    return out


def kernel_meta(text):
    """[(kernel name, scratch bytes, SGPRs, VGPRs)] from the kernels' metadata records."""
    meta = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)\n\s+\.sgpr_count:\s+(\d+)"
                      r"(?:\n.*?)*?\n\s+\.vgpr_count:\s+(\d+)", text)
    return [(n, int(scratch), int(sgpr), int(vgpr)) for n, scratch, sgpr, vgpr in meta]


def reads_register(ins, reg):
    """Does instruction text `ins` mention VGPR number `reg` (alone or inside a v[a:b] range)?"""
    for m in re.finditer(r"\bv(\d+)\b", ins):
        if int(m.group(1)) == reg:
            return True
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", ins):
        if int(m.group(1)) <= reg <= int(m.group(2)):
            return True
    return False


def check_rsq_wait_states(name, body):
    """Every v_rsq_f32 of `body` keeps the wait state gfx950 needs before its consumer; returns how many there are."""
    total = 0
    for i, ins in enumerate(body):
        if not ins.startswith("v_rsq_f32"):
            continue
        total += 1
        dest = int(re.match(r"v_rsq_f32(?:_e\d+)?\s+v(\d+)", ins).group(1))
        nxt = body[i + 1]
        assert not (nxt.startswith("v_") and reads_register(nxt, dest)), \
            f"{name}: `{ins}` is read by the very next instruction `{nxt}` (no wait state)"
        # the shipped bodies: one rsq (K = 1) or two back to back (K = 2) inside a raised-priority window whose
        # closing s_setprio 0 is the wait state before the first dependent multiply
        assert any(x.startswith("s_setprio 0") for x in body[i + 1:i + 3]), f"{name}: no s_setprio 0 after `{ins}`: {body[i + 1:i + 3]}"
        assert any(x.startswith("s_setprio 3") for x in body[i - 2:i]), f"{name}: rsq not issued at raised priority: {body[i - 2:i]}"
        reader = next(j for j in range(i + 1, len(body)) if body[j].startswith("v_") and reads_register(body[j], dest))
        assert any(x.startswith("s_") for x in body[i + 1:reader]), f"{name}: no scalar slot between `{ins}` and `{body[reader]}`"
    return total
