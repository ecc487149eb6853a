"""Energy / momentum / potential diagnostics (include/nbody_diag.h) without a GPU: the host path of GetWorldEnergy /
GetWorldPotential against a float64 numpy restatement of the definitions, the header / binding / export agreement, and
static checks on the ISA of nbody_amd/csrc/diagnostics.hip."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
from energy_ref import assert_energy_close, energy_f64, phi_f64
from gpu_common import synth

ROOT = nb.ROOT
HIPCC = "/opt/rocm/bin/hipcc"


def host_world(a):
    """A CPU-only World (never touches a device) and its partitioned particles."""
    w = nb.World(a)
    p = w.particles()
    return w, p, int(np.count_nonzero(p[:, 6] > 0))


def check_against_f64(a):
    w, p, m = host_world(a)
    phi = w.potential()
    e = w.energy()
    w.close()
    want_phi = phi_f64(p, m)
    # the host path computes Phi in float64 and rounds once to float32
    assert np.all(np.abs(phi.astype(np.float64) - want_phi) <= 6e-8 * np.abs(want_phi) + 1e-300)
    want, scale = energy_f64(p, m)
    assert_energy_close(e, want, scale)
    return p, m, phi, e


def fixture_cases():
    return ["ic_333.bin", "ic_1024.bin", "ic_4096.bin"]


@pytest.mark.parametrize("name", fixture_cases())
def test_host_path_matches_f64_on_fixtures(golden, name):
    check_against_f64(golden(name))


@pytest.mark.parametrize("n", [1, 2, 63, 65, 257, 4096])
def test_host_path_matches_f64_on_synthetic_worlds(n):
    part, _ = synth(n, seed=n)
    check_against_f64(part)


def test_host_potential_in_float64_before_the_final_rounding(golden):
    """Phi_i within 1e-12 relative: the World's float32 Phi is the float64 sum rounded once (checked through the
    energy, whose potential is the float64 sum of m_i Phi_i with Phi_i never rounded)."""
    w, p, m = host_world(golden("ic_1024.bin"))
    e = w.energy()
    w.close()
    phi = phi_f64(p, m, np.arange(m))
    want = 0.5 * np.sum(p[:m, 6].astype(np.float64) * phi)
    assert abs(e["potential"] - want) <= 1e-12 * abs(want)


def test_all_massless_world_has_potential_zero_and_no_energy():
    a = synth(300, frac_massive=0.0, seed=3)[0]
    a[:, 6] = 0.0
    w, p, m = host_world(a)
    assert m == 0
    phi, e = w.potential(), w.energy()
    w.close()
    assert np.all(phi == 0.0)       # no sources: Phi = 0 for every receiver
    assert e["kinetic"] == 0.0 and e["potential"] == 0.0 and e["mass"] == 0.0
    assert e["center_of_mass"] == (0.0, 0.0)


def test_massless_receivers_feel_the_potential():
    a = synth(200, frac_massive=0.3, seed=5)[0]
    w, p, m = host_world(a)
    phi = w.potential()
    w.close()
    assert 0 < m < p.shape[0]
    assert np.all(phi[m:] < 0.0)    # Phi != 0 for massless receivers; they add nothing to the energy
    np.testing.assert_allclose(phi[m:], phi_f64(p, m, np.arange(m, p.shape[0])), rtol=6e-8)


def two_body(m=1000.0, d=20.0, r=0.25):
    """Equal masses and radii on a circular orbit about their centre of mass: v^2 = G m d / (2 (d^2 + r)^(3/2))."""
    g = float(np.float32(nb.NB_G))
    v = np.sqrt(g * m * d / (2.0 * (d * d + r) ** 1.5))
    a = np.zeros((2, 8), dtype=np.float32)
    a[0, 0], a[1, 0] = -d / 2, d / 2
    a[0, 3], a[1, 3] = -v, v
    a[:, 6], a[:, 7] = m, r
    return a


def test_two_body_analytic():
    a = two_body()
    w, p, m = host_world(a)
    e, phi = w.energy(), w.potential()
    w.close()
    g, mass, r = float(np.float32(nb.NB_G)), float(p[0, 6]), float(p[0, 7])
    d = float(p[1, 0]) - float(p[0, 0])
    v = float(p[1, 3])
    u = -g * mass * mass / np.sqrt(d * d + r)
    assert abs(e["potential"] - u) <= 1e-12 * abs(u)
    assert abs(e["kinetic"] - 0.5 * 2 * mass * v * v) <= 1e-12 * mass * v * v
    assert e["momentum"] == (0.0, 0.0)
    np.testing.assert_allclose(phi, [-g * mass / np.sqrt(d * d + r)] * 2, rtol=1e-7)


def core_plus_particles(n=512, seed=7):
    """A heavy core with a tiny radius among light particles far away: the core's self term G m / sqrt(r) is ~10^6 x the
    rest of its sum, so a Phi that subtracted it afterwards would keep no correct digit in float32."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 1.0e3 + 5.0e3
    a[:, 6], a[:, 7] = 1.0, 1.0
    a[0, 0:2] = 0.0
    a[0, 6], a[0, 7] = 1.0e6, 1.0e-4
    return a


def test_self_term_is_excluded_by_index():
    w, p, m = host_world(core_plus_particles())
    phi = w.potential()
    w.close()
    core = int(np.argmax(p[:, 6]))
    want = phi_f64(p, m, np.array([core]))[0]
    self_term = float(np.float32(nb.NB_G)) * float(p[core, 6]) / np.sqrt(float(p[core, 7]))
    assert self_term > 1e5 * abs(want)
    assert abs(float(phi[core]) - want) <= 1e-7 * abs(want)


def test_host_result_does_not_depend_on_the_thread_count(tmp_path):
    code = ("import sys, hashlib, numpy as np, nbody_amd as nb\n"
            "sys.path.insert(0, 'tests')\n"
            "from gpu_common import synth\n"
            "w = nb.World(synth(3000, seed=11)[0]); e = w.energy(); phi = w.potential()\n"
            "sys.stdout.write(repr([e['kinetic'], e['potential'], e['angular_momentum'], list(e['momentum'])]) + ' ' + "
            "hashlib.sha256(phi.tobytes()).hexdigest())\n")
    outs = []
    for threads in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]


def test_cpu_only_world_never_opens_a_device(tmp_path):
    """GetWorldEnergy / GetWorldPotential of a World that only stepped on the CPU run on the host: no device is opened
    (on a box without a GPU any device contact aborts, test_gpu_call_without_gpu_aborts_loudly)."""
    code = ("import os, numpy as np, nbody_amd as nb\n"
            "a = np.zeros((64, 8), dtype=np.float32); a[:, 0] = np.arange(64); a[:, 6] = 1; a[:, 7] = 1\n"
            "w = nb.World(a); w.update_cpu(0.01, 2); e = w.energy(); phi = w.potential(); w.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', e['potential'] < 0, bool(np.all(phi < 0)))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["OK", "True", "True"]


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", text, re.M)


def exported(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_diag_header_binding_and_exports_agree():
    assert set(declared_functions("nbody_diag.h")) == {"GetWorldEnergy", "GetWorldPotential"}
    assert {"GetWorldEnergy", "GetWorldPotential"} <= set(nb.NBODY_API)
    assert {"GetWorldEnergy", "GetWorldPotential"} <= exported(nb.NBODY_SO)
    assert {"nb_hip_energy", "nb_hip_potential"} <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API)
    assert {"nb_hip_energy", "nb_hip_potential"} <= exported(nb.HIP_SO)
    assert not {"nb_cpu_energy", "nb_cpu_potential"} & exported(nb.NBODY_SO)   # the host path is internal
    assert nb.hip_lib().nb_hip_version() == 400
    # the struct as C lays it out
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "nbody_hip.h"\n'
           'int main(void){ printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(WorldEnergy), offsetof(WorldEnergy, potential), '
           'offsetof(WorldEnergy, mass), offsetof(WorldEnergy, momentum), offsetof(WorldEnergy, angular_momentum), '
           'offsetof(WorldEnergy, center_of_mass)); return 0; }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o",
                        os.path.join(d, "t")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.split()]
    E = nb.WorldEnergy
    assert out == [C.sizeof(E), E.potential.offset, E.mass.offset, E.momentum.offset, E.angular_momentum.offset,
                   E.center_of_mass.offset]


def test_diag_functions_stay_out_of_the_reference_headers():
    for h in ("nbody.h", "galaxy.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "GetWorldEnergy" not in text and "GetWorldPotential" not in text


def test_sharded_world_energy_aborts_with_a_clear_message():
    code = ("import nbody_amd as nb, numpy as np, ctypes as C\n"
            "a = np.zeros((16, 8), dtype=np.float32); a[:, 0] = np.arange(16); a[:, 6] = 1; a[:, 7] = 1\n"
            "L = nb.nbody_lib(); fn = nb.ALLGATHER_FN(lambda *x: None)\n"
            "w = L.CreateWorldShardedWith(a.ctypes.data, 16, 0, 2, fn, None)\n"
            "e = nb.WorldEnergy(); L.GetWorldEnergy(w, C.byref(e)); print('SURVIVED')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout
    assert re.search(r"\.c:\d+ \[\w+\]", r.stderr) and "sharded pipeline needs a collective" in r.stderr, r.stderr


# ---- static ISA of diagnostics.hip ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def diag_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    make = open(os.path.join(ROOT, "nbody_amd", "csrc", "Makefile")).read()
    flags = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17"]
    line = re.search(r"^HIPFLAGS\s*:=(.*)$", make, re.M).group(1)
    assert all(f.replace("gfx950", "$(ARCH)") in line for f in flags)   # the Makefile's flags
    assert re.search(r"^HIP_TUS\s*:=.*\bdiagnostics\b", make, re.M)
    out = tmp_path_factory.mktemp("diag_isa") / "diagnostics.s"
    cmd = [HIPCC] + flags + ["-Wno-unused-command-line-argument", f"-I{ROOT}/include", f"-I{ROOT}/nbody_amd/csrc",
                             "--cuda-device-only", "-S", "-o", str(out), os.path.join(ROOT, "nbody_amd", "csrc", "diagnostics.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out.read_text()


def kernel_metadata(text):
    """kernel symbol -> {vgpr_count, private_segment_fixed_size, ...} from the amdhsa metadata."""
    out = {}
    for block in re.split(r"\n\s+- \.", text.split("amdhsa.kernels:")[1]):
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def basic_blocks(text, symbol):
    body = text[text.index(symbol + ":"):]
    body = body[:body.index(".Lfunc_end")]
    parts = re.split(r"^(\.LBB\d+_\d+):", body, flags=re.M)
    for k in range(1, len(parts), 2):
        lines = [ln.split(";")[0].strip() for ln in parts[k + 1].splitlines()]
        ins = [ln for ln in lines if ln and not ln.startswith(".")]
        yield parts[k], ins


def test_diagnostics_kernels_have_no_scratch_and_keep_their_vgpr_budget(diag_isa):
    meta = kernel_metadata(diag_isa)
    names = set(meta)
    assert any("potential_kernel" in n for n in names) and any("energy_reduce_kernel" in n for n in names), names
    assert not any("step_kernel" in n for n in names)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, name
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, name
        # potential_kernel: __launch_bounds__(512, 8) = eight waves per SIMD -> at most 64 VGPRs
        if "potential_kernel" in name:
            assert m["vgpr_count"] <= 64, m
            assert m["max_flat_workgroup_size"] == 512


def test_diagnostics_write_memory_with_vector_stores_only(diag_isa):
    ops = {ln.split()[0] for ln in diag_isa.splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))}
    writes = {op for op in ops if "store" in op or "atomic" in op}
    assert writes and all(op.startswith(("global_", "ds_", "buffer_", "flat_")) for op in writes), writes


def test_potential_loop_is_five_valu_and_one_rsq_per_pair(diag_isa):
    sym = next(n for n in kernel_metadata(diag_isa) if "potential_kernel" in n)
    loops = []
    for label, ins in basic_blocks(diag_isa, sym):
        ops = [i.split()[0] for i in ins]
        if any(label in i for i in ins if i.startswith("s_cbranch") or i.startswith("s_branch")) and "v_rsq_f32" in " ".join(ops):
            loops.append((label, ops))
    plain = [(lab, ops) for lab, ops in loops if not any(o.startswith("v_cndmask") for o in ops)]
    masked = [(lab, ops) for lab, ops in loops if any(o.startswith("v_cndmask") for o in ops)]
    assert plain and masked, loops   # the off-diagonal loop and the diagonal block's masked loop are separate
    big = max(plain, key=lambda x: x[1].count("v_rsq_f32"))
    ops = big[1]
    rsq = sum(o.startswith("v_rsq_f32") for o in ops)
    other = [o for o in ops if o.startswith("v_") and not o.startswith("v_rsq_f32")]
    assert rsq == 16, big              # 8 sources x 2 receivers per lane
    assert len(other) <= 5 * rsq, (len(other), sorted(set(other)))
    assert not [o for o in other if o.startswith("v_pk_")], other
    # sources arrive through the scalar cache, never as vector loads inside the loop
    assert "s_load_dwordx16" in ops and "s_load_dwordx8" in ops
    assert not [o for o in ops if o.startswith(("global_load", "buffer_load", "flat_load"))]
    # gfx950: one wait state between v_rsq_f32 and the instruction that reads its result
    for i, o in enumerate(ops):
        if o.startswith("v_rsq_f32"):
            assert ops[i + 1].startswith("s_"), ops[i:i + 3]
