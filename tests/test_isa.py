"""Static checks on the gfx950 ISA of the step kernels (no GPU needed: hipcc cross-compiles).

The hot loop is hand-written asm (nbody_amd/csrc/kernels.hip, NB_INTERACTION_ASM) and leans on three invariants that
only the GPU parity tests would otherwise notice:
  1. gfx950 needs one wait state between a transcendental (v_rsq_f32) and the VALU instruction that reads its
     result, and hipcc cannot pad inside an asm statement: the `s_setprio 0` that follows the rsq IS that wait state
     (round 1 shipped-then-fixed a variant without it that read stale values);
  2. every step kernel must stay within 64 VGPRs, or a 1024-thread workgroup no longer fits twice on a CU
     (__launch_bounds__(1024, 8));
  3. no scratch: a spill inside the inner loop would sit on the critical path.
"""
import os
import re
import struct

import pytest

from isa_common import ROOT, check_rsq_wait_states, compile_isa, functions, kernel_meta


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("isa"), "kernels.hip")


@pytest.fixture(scope="module")
def convert_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("convert_isa"), "convert.hip")


def test_every_rsq_has_a_wait_state_before_its_consumer(isa):
    fns = {n: body for n, body in functions(isa).items() if "step_kernel" in n}
    assert len(fns) >= 16, sorted(fns)
    total = sum(check_rsq_wait_states(name, body) for name, body in fns.items())
    assert total >= 16 * 8, total


def test_step_kernel_instantiations_fit_the_occupancy_the_launch_bounds_promise(isa):
    step = [row for row in kernel_meta(isa) if "step_kernel" in row[0]]
    assert len(step) >= 16
    for name, scratch, sgpr, vgpr in step:
        assert vgpr <= 64, f"{name}: {vgpr} VGPRs (> 64 halves the occupancy of a 1024-thread workgroup)"
        assert scratch == 0, f"{name}: {scratch} bytes of scratch (spills)"
        assert sgpr <= 102, f"{name}: {sgpr} SGPRs"
    # the default (scalar-cache) route keeps the asm body's footprint: well under the limit
    # (template arguments: K, W, VARIANT = 1, FUSED)
    smem = [v for n, _, _, v in step if re.search(r"ELi1ELb[01]EEEvNS_10StepParamsE$", n)]
    assert len(smem) >= 14 and max(smem) <= 48, smem


def test_interaction_body_is_the_twelve_instruction_sequence(isa):
    """One (source, receiver) interaction = 2 x v_sub, v_fma, v_fmac, s_setprio, v_rsq, s_setprio, 3 x v_mul, 2 x v_fmac
    in their short encodings (the 8-byte VOP3 forms measured 11.6 % slower); with two receivers per lane the two
    interactions of a source share one priority window; and NO packed f32 instruction in the step kernels' loops
    (v_pk_add / v_pk_fma around the transcendental cost 4.5 %: DESIGN.md section 3)."""
    head = ["v_sub_f32", "v_sub_f32", "v_fma_f32", "v_fmac_f32"]
    tail = ["v_mul_f32", "v_mul_f32", "v_mul_f32", "v_fmac_f32", "v_fmac_f32"]
    single = head + ["s_setprio", "v_rsq_f32", "s_setprio"] + tail                       # K = 1
    paired = head + head + ["s_setprio", "v_rsq_f32", "v_rsq_f32", "s_setprio"] + tail + tail   # K = 2: both receivers of a lane
    for kernel, want, least in (("step_kernelILi1ELi16ELi1E", single, 16), ("step_kernelILi2ELi16ELi1E", paired, 16)):
        body = next(b for n, b in functions(isa).items() if kernel in n)
        ops = [ins.split()[0] for ins in body]
        hits = sum(1 for i in range(len(ops) - len(want) + 1) if ops[i:i + len(want)] == want)
        assert hits >= least, (kernel, hits)      # two unrolled 8-source groups at least
    assert not any(op.endswith("_e64") for op in ops if op.startswith(("v_mul_f32", "v_fmac_f32", "v_rsq_f32", "v_sub_f32")))
    # between one v_rsq_f32 and the next (one interaction's tail, the next one's head) nothing packed may appear
    rsq = [i for i, op in enumerate(ops) if op == "v_rsq_f32"]
    for a, b in zip(rsq, rsq[1:]):
        if b - a <= 14:
            assert not any(op.startswith("v_pk_") for op in ops[a:b]), ops[a:b]


def test_the_gravitational_constant_is_written_down_once(convert_isa):
    """NB_G lives in include/nbody.h and nowhere else: the kernels get it as a launch argument from the host, like the
    reference's specialisation constant (reference src/lib/sim_gpu.c:54-72, src/shader/particle_cs.glsl:26).  No source
    under nbody_amd/csrc may spell the value, and the device code of the kernels that multiply by G (convert.hip: exactly the
    callers of g_times_m) must not hold it as an instruction literal either."""
    header = open(os.path.join(ROOT, "include", "nbody.h")).read()
    value = float(re.search(r"^#define\s+NB_G\s+([0-9.eE+-]+)f\s*$", header, re.M).group(1))
    literal = "0x%08x" % struct.unpack("<I", struct.pack("<f", value))[0]          # 0x41200000 for 10.0f
    spelled = re.compile(r"(?<![\w.])%s(?:\.0*)?f?(?![\w.])" % re.escape(("%g" % value)))
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h", ".c")) or name in ("galaxy.c", "bench_main.c"):
            continue    # galaxy.c / bench_main.c: host code with unrelated tens (radii, warm-up steps); they use NB_G by name
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(csrc, name)).read(), flags=re.S)
        for m in spelled.finditer(text):
            line = text[text.rfind("\n", 0, m.start()) + 1:text.find("\n", m.end())]
            assert not re.search(r"f\b", m.group(0)) and "mul" not in line, f"{name}: `{line.strip()}` spells NB_G's value"
    for src in ("kernels.hip", "convert.hip", "launch_shape.hip", "pipeline.hip"):
        assert "10.0f" not in open(os.path.join(csrc, src)).read(), src
    assert "NB_G" in open(os.path.join(csrc, "pipeline.hip")).read()
    # the kernels that multiply by G are exactly the ones that call the shared helper, and nothing outside convert.hip does
    text = open(os.path.join(csrc, "convert.hip")).read()
    callers = set()
    for m in re.finditer(r"__global__ void (\w+)\(.*?\n}\n", text, flags=re.S):
        if "g_times_m(" in m.group(0):
            callers.add(m.group(1))
    assert callers == {"make_gm_kernel", "split_sources_kernel", "batch_split_kernel"}, callers
    assert len(re.findall(r"\bg_times_m\(", text)) == len(callers) + 1                    # one definition, one call each
    assert not [n for n in sorted(os.listdir(csrc)) if n != "convert.hip" and "g_times_m" in open(os.path.join(csrc, n), errors="replace").read()]
    fns = functions(convert_isa)
    multiply = {n for n, b in fns.items() if any(ins.startswith(("v_mul_f32", "v_pk_mul_f32")) for ins in b)}
    users = {n: b for n, b in fns.items() if any(c in n for c in callers)}
    # batch_split_kernel is built twice: for the members of a uniform and of a ragged ensemble
    assert len(users) == 4 and sum("batch_split_kernel" in n for n in users) == 2 and set(users) == multiply, (sorted(users), sorted(multiply))
    for name, body in users.items():
        assert any(ins.startswith("v_mul_f32") for ins in body), name
        assert not any(literal in ins.lower() or re.search(r"\b10\.0\b", ins) for ins in body), (name, literal)


def test_the_shipped_build_holds_exactly_the_picked_step_kernels(isa):
    """The step_kernel instantiations of the shipped build are exactly the ones kernels.hip pick / pick_fused enumerate:
    both routes at K = 1, 2 and W = 1, 4, 8, 16, plus the six fused-finish ones (scalar-cache route, W >= 4).  The tuning-only
    shapes (K = 4, W = 2) exist in make TUNING=1 builds only."""
    shipped = {(k, w, v, 0) for v in (0, 1) for k in (1, 2) for w in (1, 4, 8, 16)}
    shipped |= {(k, w, 1, 1) for k in (1, 2) for w in (4, 8, 16)}
    built = set()
    for n in functions(isa):
        if "step_kernel" in n:
            # template arguments <K, W, VARIANT, FUSED>
            m = re.search(r"step_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EEEvNS_10StepParamsE$", n)
            assert m, n
            built.add(tuple(int(x) for x in m.groups()))
    assert built == shipped, sorted(built ^ shipped)


def test_fused_finish_tail_uses_agent_scope_accesses_and_leaves_the_unfused_kernels_alone(isa):
    """The fused-finish instantiations (step_kernel<K, W, SMEM, true>) hand the parts over with agent-scope accesses: one
    8-byte `sc1` store per receiver, a wait for the workgroup's own stores before the ticket (`global_atomic_add` with
    return), sixteen 8-byte `sc1` loads issued back to back in the last arriver's tail -- and no fence (`buffer_wbl2` /
    `buffer_inv`, the L2 write-back that made round 1's first version 5-13x slower).  The unfused instantiations contain
    none of it: their code is what it was."""
    fn = functions(isa)
    # template arguments <K, W, VARIANT, FUSED>: ...ELi<K>ELi<W>ELi<VARIANT>ELb<FUSED>EEEv
    fused = {n: b for n, b in fn.items() if "step_kernel" in n and re.search(r"Lb1EEEv", n)}
    plain = {n: b for n, b in fn.items() if "step_kernel" in n and re.search(r"Lb0EEEv", n)}
    assert len(fused) == 6 and len(plain) >= 16
    for name, body in fused.items():
        text = "\n".join(body)
        assert len(re.findall(r"global_store_dwordx2 .* sc1", text)) >= 1, name
        assert len(re.findall(r"global_load_dwordx2 .* sc1", text)) >= 16, name
        atom = [i for i, x in enumerate(body) if x.startswith("global_atomic_add")]
        assert len(atom) == 1 and "sc0" in body[atom[0]], name                        # the ticket, with its return value
        # order on the way to the ticket: the part store, a wait for it, the workgroup barrier, then the atomic
        store = max(i for i, x in enumerate(body[:atom[0]]) if re.match(r"global_store_dwordx2 .* sc1", x))
        wait = next(i for i in range(store + 1, atom[0]) if body[i].startswith("s_waitcnt vmcnt(0)"))
        assert any(x.startswith("s_barrier") for x in body[wait + 1:atom[0]]), name
        assert "buffer_wbl2" not in text and "buffer_inv" not in text, name
    for name, body in plain.items():
        text = "\n".join(body)
        assert "global_atomic" not in text and not re.search(r"global_(load|store)\S* .* sc1", text), name


def test_the_launch_policy_holds_no_device_code(tmp_path):
    """launch_shape.hip is host arithmetic only: its device-side compilation emits no kernel and no device function, so
    policy edits cannot move the kernel-source hash (benchlib.KERNEL_SOURCES) and kernels cannot hide outside it."""
    text = compile_isa(tmp_path, "launch_shape.hip")
    assert ".amdhsa_kernel" not in text and "s_endpgm" not in text and "s_setpc_b64" not in text, text[:2000]
    assert not functions(text)
    assert not re.findall(r"^\s*[vs]_\w+", text, flags=re.M)        # not one instruction
    # and the three hashed files hold no launch policy in return
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    hashed = "".join(open(os.path.join(csrc, n)).read() for n in ("kernels.hip", "kernels.h", "interaction_asm.h"))
    assert "NB_HASH_O" not in hashed
    for name in ("small_launch_cost_us", "choose_shape(LaunchShape want", "struct LaunchShape {"):
        assert name not in hashed, name
