"""The C-ABI boundary without a GPU: libraries load, export what include/*.h declares, host-only calls work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nbody_amd as nb

ROOT = nb.ROOT
FUNC = re.compile(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", re.M)


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)          # comments
    text = re.sub(r"static inline[^{]*\{[^}]*\}", "", text)     # inline helpers are not exports
    text = re.sub(r"typedef[^;{]*\(\s*\*\s*\w+\s*\)\s*\([^;]*\);", "", text)   # function-pointer typedefs are not exports
    names = [m.group(1) for m in FUNC.finditer(text)]
    return [n for n in names if n not in ("defined", "static_assert", "_Static_assert")]


def exported(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_hip_library_exports_every_declared_symbol():
    names = declared_functions("nbody_hip.h")
    assert {"CreateSimPipeline", "DestroySimPipeline", "GetSimulationData", "SetSimulationData",
            "PerformSimUpdate"} <= set(names)      # the reference seam, src/lib/sim_gpu.h:21-36
    have = exported(nb.HIP_SO)
    missing = [n for n in names if n not in have]
    assert not missing, f"libnbody_hip.so lacks {missing}"
    assert set(names) == set(nb.HIP_API), "python binding and header disagree"


def test_tuning_hooks_are_exported_but_not_part_of_the_public_header():
    """ABI 0.3.0: launch-shape and experiment knobs left include/nbody_hip.h.  They live on as test /
    tooling hooks declared in nbody_amd/csrc/nbody_hip_tuning.h: the library exports them, the public header does not
    mention them, and nb_hip_configure's documentation lists exactly the five knobs a user of the reference harness needs."""
    public = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    have = exported(nb.HIP_SO)
    tuning = open(os.path.join(ROOT, "nbody_amd", "csrc", "nbody_hip_tuning.h")).read()
    for name in nb.TUNE_API:
        assert name in have and re.search(r"\b%s\s*\(" % name, tuning), name
        assert not re.search(r"\b%s\s*\(" % name, public), f"{name} is declared in the public header"
    doc = public[public.index("Run-time knobs"):public.index("int nb_hip_configure")]
    assert re.findall(r'^ \*   "(\w+)"', doc, flags=re.M) == list(nb.PUBLIC_KNOBS)
    assert nb.hip_lib().nb_hip_version() >= 300
    # the environment presets of the shipped library: the documented ones only (the rest exist in TUNING=1 builds)
    src = open(os.path.join(ROOT, "nbody_amd", "csrc", "pipeline.hip")).read()
    shipped = src.split("#ifdef NB_TUNING_SHAPES")[0]
    assert set(re.findall(r'getenv\("(NB_HIP_\w+)"\)', shipped)) == {"NB_HIP_VARIANT", "NB_HIP_GRAPH"}


def test_nbody_library_exports_public_surface():
    names = declared_functions("nbody.h") + declared_functions("galaxy.h")
    assert set(names) == {"CreateWorld", "DestroyWorld", "GetWorldParticles", "UpdateWorld_CPU",
                          "UpdateWorld_GPU", "MakeGalaxies",   # reference nbody.h:61-73, galaxy.h:64
                          "MakeGalaxiesSeeded",                # extension: libc-independent draws
                          "CreateWorldSharded",                # extension: one World per process and GPU
                          "CreateWorldShardedWith",            # ... over a caller-supplied host all-gather
                          "CreateWorldShardedDirect",          # ... over direct device-to-device pushes (IPC-mapped peers)
                          "GetWorldPipeline"}                  # extension: the pipeline behind a World (knobs, timers)
    have = exported(nb.NBODY_SO)
    assert not [n for n in names if n not in have]


def test_libraries_load_and_bind():
    nb.nbody_lib()
    assert nb.hip_lib().nb_hip_version() >= 100
    assert nb.device_count() >= 0  # never aborts, also without a GPU


def test_hip_library_does_not_link_oracle_or_rccl_eagerly():
    out = subprocess.run(["ldd", nb.HIP_SO], check=True, capture_output=True, text=True).stdout
    assert "oracle" not in out and "librccl" not in out
    out = subprocess.run(["ldd", nb.NBODY_SO], check=True, capture_output=True, text=True).stdout
    assert "oracle" not in out


def test_particle_layout_is_32_bytes():
    src = r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "nbody.h"
    #include "nbody_hip.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(Particle), offsetof(Particle,pos), offsetof(Particle,vel),
      offsetof(Particle,acc), offsetof(Particle,mass), offsetof(Particle,radius), sizeof(WorldData)); return 0; }'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o",
                        os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["32", "0", "8", "16", "24", "28", "12"]   # reference nbody.h:47-55, sim_gpu.h:8-12


def test_pipeline_create_destroy_needs_no_gpu():
    L = nb.hip_lib()
    h = L.CreateSimPipeline(nb.WorldData(1000, 400, 0.0))
    assert h
    L.DestroySimPipeline(h)
    L.DestroySimPipeline(None)   # NULL accepted, reference sim_gpu.c:224


def test_live_resources_are_even_across_create_destroy_without_a_gpu():
    """nb_hip_live_resources counts what the owner types hold: an object that never reached the device takes nothing and
    gives nothing back, and deleting it makes no HIP call (this runs with no device present)."""
    L = nb.hip_lib()
    base = nb.live_resources()
    L.DestroySimPipeline(L.CreateSimPipeline(nb.WorldData(1000, 400, 0.0)))
    assert nb.live_resources() == base
    mass = (C.c_uint32 * 3)(120, 0, 250)
    L.nb_hip_batch_destroy(L.nb_hip_batch_create(3, 250, mass))
    assert nb.live_resources() == base
    sizes, mass = (C.c_uint32 * 3)(100, 600, 2000), (C.c_uint32 * 3)(50, 300, 1000)   # one member per launch group
    L.nb_hip_batch_destroy(L.nb_hip_ragged_create(3, sizes, mass))
    assert nb.live_resources() == base


@pytest.mark.parametrize("N,M,P", [(1 << 20, 523884, 8), (1 << 20, 523884, 2), (4096, 1989, 4), (333, 150, 8),
                                   (100, 0, 3), (100, 100, 3), (65, 1, 2), (0, 0, 2), (1 << 22, 2100000, 8)])
def test_shard_plan_covers_everything_once(N, M, P):
    plans = [nb.shard_plan(N, M, r, P) for r in range(P)]
    mc, zc = plans[0]["mass_chunk"], plans[0]["zero_chunk"]
    assert all(p["mass_chunk"] == mc and p["zero_chunk"] == zc and p["src_padded"] == P * mc for p in plans)
    assert mc % 64 == 0 and zc % 64 == 0           # wave-aligned, uniform all-gather counts / allocations
    owned = np.zeros(N, dtype=np.int32)
    for r, p in enumerate(plans):
        assert p["mass_count"] <= mc and p["zero_count"] <= zc
        if p["mass_count"]:
            assert p["mass_begin"] == r * mc       # gathered index == global massive index
        assert p["mass_begin"] + p["mass_count"] <= M
        assert M <= p["zero_begin"] and p["zero_begin"] + p["zero_count"] <= N
        owned[p["mass_begin"]:p["mass_begin"] + p["mass_count"]] += 1
        owned[p["zero_begin"]:p["zero_begin"] + p["zero_count"]] += 1
    assert np.all(owned == 1)
    # balance: every receiver costs the same, so per-rank totals are levelled: ranks whose massive slice alone
    # is not above the level differ by at most one receiver
    totals = [p["mass_count"] + p["zero_count"] for p in plans]
    levelled = [t for t, p in zip(totals, plans) if p["zero_count"] > 0]
    if levelled:
        assert max(levelled) - min(levelled) <= 1
        assert all(p["mass_count"] >= max(levelled) - 1 for p in plans if p["zero_count"] == 0)
    assert sum(totals) == N
    assert all(p["zero_count"] <= zc for p in plans)


def test_shard_plan_bench_case_lands_on_round_boundaries():
    # N = 2^20, the BASELINE universe: every rank gets exactly N/P receivers -> 1024-thread workgroups of
    # 128 receivers fill whole rounds of the 512 resident slots
    for P in (2, 4, 8):
        for r in range(P):
            p = nb.shard_plan(1 << 20, 523884, r, P)
            assert p["mass_count"] + p["zero_count"] == (1 << 20) // P


def test_launch_plan_round_boundaries_and_splits():
    # 256 CUs, two 1024-thread workgroups resident per CU = 512 slots per round
    for n, m in ((1 << 20, 523884), (262144, 130916), (131072, 262144)):
        p = nb.plan_launch(n, m)
        # large grids: K = 2, W = 16, whole rounds; a modest split keeps the launch's ragged end small
        assert (p["k"], p["w"]) == (2, 16) and 1 <= p["split"] <= 8
        assert p["workgroups"] == n // 128 * p["split"] and p["workgroups"] % 512 == 0
    # config 2 (N = 65 536): exactly two rounds of 1024-thread workgroups either way; with the plain interaction body one
    # receiver per lane costs 1.6 % more than two, so the single-kernel unsplit shape wins (395 vs 394 us measured)
    p = nb.plan_launch(65536, 32641)
    assert p["w"] == 16 and p["workgroups"] == 1024 and (p["k"], p["split"]) in ((1, 1), (2, 2))
    for n, m in ((100000, 49944), (200000, 99899)):
        p = nb.plan_launch(n, m)
        assert p["split"] > 1 and p["workgroups"] == -(-n // (64 * p["k"])) * p["split"]    # off a boundary: split
        rounds = -(-p["workgroups"] // (256 * 32 // p["w"]))
        assert p["workgroups"] / (rounds * 256 * 32 // p["w"]) > 0.9                          # last round nearly full
    for n, m in ((250, 119), (500, 244), (800, 386)):
        p = nb.plan_launch(n, m)
        # a handful of tiles: unsplit, 16 waves on each -- 8 while there are no more than 128 sources -- and fine granules
        assert (p["k"], p["w"], p["split"]) == (1, 8 if m <= 128 else 16, 1) and p["unit"] < 64
    assert nb.plan_launch(20000, 9956)["split"] > 1                                         # unsplit: 69 us, split: 45 us
    for n, m in ((2000, 967), (3000, 1467), (4096, 1989), (6000, 2957), (10000, 4917)):
        p = nb.plan_launch(n, m)
        # latency-bound: every wave's serial chain is cut short by splitting the sources over many small workgroups
        # (N = 4000: 10.4 us unsplit with 1024-thread workgroups, 6.8 us with 8 parts of 256- or 512-thread ones)
        assert p["w"] in (4, 8) and 4 <= p["split"] <= 16
    for n, m in ((1, 0), (1, 1), (64, 64), (0, 0), (4194304, 2100000), (123457, 7)):
        p = nb.plan_launch(n, m)
        assert p["k"] in (1, 2) and p["w"] in (4, 8, 16) and 1 <= p["split"] <= 16
    assert nb.plan_launch(1 << 20, 523884, compute_units=0)["k"] == 2                       # 0 CUs -> default 256


def test_fused_finish_rule():
    """nb_hip_plan_fused_finish: split steps run without the finish kernel from N x M >= 4e7 (where the in-kernel
    hand-over also wins inside a hipGraph, profiles/r04_fused_finish.txt) up to 200 000 receivers; unsplit and lane-split
    shapes have nothing to fuse."""
    want = {(5000, 2439): 0, (8000, 3919): 0, (10000, 4917): 1, (14000, 6911): 1, (20000, 9956): 1, (50000, 24850): 1,
            (100000, 49944): 1, (65536, 32641): 0, (262144, 130916): 0, (1 << 20, 523884): 0, (2000, 967): 0, (0, 0): 0}
    for (n, m), fused in want.items():
        assert nb.plan_launch(n, m)["fused_finish"] == fused, (n, m)


def test_lane_split_rule_matches_the_committed_scan():
    """nb_hip_plan_launch_lanes: latency-bound unsharded steps (N x M <= 9e6) run as lane-split launches -- (lanes, w) read
    off profiles/r03_lane_split_scan.txt -- and nothing above that does (the scheme loses once a step is throughput)."""
    want = {(250, 119): (4, 8), (500, 244): (4, 8), (800, 386): (8, 8), (1200, 586): (8, 8), (2000, 967): (8, 8),
            (3000, 1467): (4, 16), (4000, 1937): (4, 16)}
    for (n, m), (lanes, w) in want.items():
        p = nb.plan_launch(n, m)
        assert (p["lanes"], p["lanes_w"]) == (lanes, w), (n, m, p)
    for n, m in ((5000, 2439), (10000, 4917), (20000, 9956), (65536, 32641), (1 << 20, 523884), (100, 0), (0, 0)):
        assert nb.plan_launch(n, m)["lanes"] == 1, (n, m)
    # the committed scan really says so: at every scanned size up to N = 4 000 some lane-split shape beats the classic
    # auto shape; from N = 5 000 on none does EXCEPT the N = 6 000 row, where lanes = 4, w = 16 edges the classic pick out
    # by ~2 % while its neighbours 5 000 and 8 000 lose -- a non-monotonic row the rule's 9e6-pair cut-off deliberately
    # does not chase
    import re
    text = open(os.path.join(ROOT, "profiles", "r03_lane_split_scan.txt")).read()
    block = text[text.index("== the shipped (tiled) kernel"):text.index("== the shipped kernel (velocity")]
    rows = re.findall(r"^N=\s*(\d+) M=\s*\d+: auto\s+([\d.]+) us .*?\| lanes=\d+ w=\d+:\s+([\d.]+) us", block, re.M)
    assert len(rows) >= 10
    for n, auto_us, best_us in rows:
        assert (float(best_us) < float(auto_us)) == (int(n) <= 4000 or int(n) == 6000), (n, auto_us, best_us)


def test_gpu_call_without_gpu_aborts_loudly():
    """No CPU fallback: UpdateWorld_GPU on a box without a GPU must abort, not compute."""
    if nb.device_count() > 0:
        pytest.skip("a GPU is present")
    code = ("import numpy as np, nbody_amd as nb\n"
            "a=np.zeros((8,8),dtype=np.float32); a[:,6]=1; a[:,7]=1\n"
            "w=nb.World(a); w.update_gpu(0.1,1); print('SURVIVED')\n")
    r = subprocess.run(["python", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout
    assert "no HIP device" in r.stderr or "hipError" in r.stderr


# The reference's error convention (src/lib/util.h:17-29): no return codes; every failure prints
# `file:line [func] message` to stderr and abort()s.  Each case runs in a child process.
ERROR_CASES = [
    ("mass_len > total_len", "s = nb.SimPipeline(10, 11)", "mass_len 11 > total_len 10"),
    ("unknown knob", "s = nb.SimPipeline(10, 5); nb.hip_lib().nb_hip_configure(s._h, b'nonsense', 1)", 'unknown knob "nonsense"'),
    ("tuning hook is not a public knob", "s = nb.SimPipeline(10, 5); nb.hip_lib().nb_hip_configure(s._h, b'k', 1)", 'unknown knob "k"'),
    ("unknown tuning hook", "s = nb.SimPipeline(10, 5); s.configure(nonsense=1)", 'unknown tuning hook "nonsense"'),
    ("bad knob value", "s = nb.SimPipeline(10, 5); s.configure(k=3)", "k must be 0, 1, 2 or 4, got 3"),
    ("bad graph mode", "s = nb.SimPipeline(10, 5); s.configure(graph=7)", "graph must be 0"),
    ("update before set", "s = nb.SimPipeline(10, 5); s.update(1, 0.1)", None),
    ("get before set", "s = nb.SimPipeline(10, 5); s.get_data()", None),
    ("sharded without id", "import ctypes as C; L = nb.hip_lib(); "
     "L.CreateSimPipelineSharded(nb.WorldData(10, 5, 0.0), 0, 2, None)", "needs the RCCL unique id"),
    ("bad rank", "L = nb.hip_lib(); L.nb_hip_shard_plan(10, 5, 3, 2, None)", "rank 3 of 2"),
]


@pytest.mark.parametrize("name,code,needle", ERROR_CASES, ids=[c[0] for c in ERROR_CASES])
def test_failures_print_file_line_func_and_abort(name, code, needle):
    r = subprocess.run(["python", "-c", "import nbody_amd as nb\n" + code + "\nprint('SURVIVED')"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    # file:line [function] ...
    import re
    assert re.search(r"\.(hip|c|cpp|h):\d+ \[\w+\]", r.stderr), r.stderr
    if needle:
        assert needle in r.stderr, r.stderr


def test_small_launch_model_against_the_committed_shape_scan():
    """profiles/r02_sweep_shapes_units.txt is the exhaustive (K, W, split, unit) scan the small-launch cost model was
    fitted on (3 360 timed shapes, MI355X).  The model's pick for each scanned size must stay close to the scan's best:
    a change to choose_shape that loses more than 6 % at any size, or 2.5 % on average, is a regression."""
    path = os.path.join(ROOT, "profiles", "r02_sweep_shapes_units.txt")
    rows = np.loadtxt(path)                     # N M K W split unit workgroups us_per_step
    regrets = []
    for n in sorted(set(rows[:, 0])):
        sub = rows[rows[:, 0] == n]
        m = int(sub[0, 1])
        p = nb.plan_launch(int(n), m)
        hit = sub[(sub[:, 2] == p["k"]) & (sub[:, 3] == p["w"]) & (sub[:, 4] == p["split"]) & (sub[:, 5] == p["unit"])]
        if len(hit) == 0:
            continue    # the scan covers splits 1-6, 8, 10, 13, 16; a pick in between (9 at N = 14 000: 990 workgroups,
                        # one round of 1024 slots, 25.2 us on the GPU against the scan's best 25.5) cannot be priced here
        regrets.append(hit[0, 7] / sub[:, 7].min() - 1.0)
        assert regrets[-1] <= 0.06, f"N={int(n)}: pick {p} measured {hit[0, 7]} us, scan's best {sub[:, 7].min()} us"
    assert len(regrets) >= 12
    assert np.mean(regrets) <= 0.025, regrets


# ---- nbody-bench --gpus P: the shared rank page (rank_page.c), no GPU involved -------------------------------------------

BENCH_EXE = os.path.join(nb.LIB_DIR, "nbody-bench")


@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_rank_page_selftest_with_real_processes(P):
    """P forked processes meet at barriers, pass three 128-byte ids from rank 0, reduce max / min / sum, compare words and
    run 250 shared-memory all-gathers of 4 B .. 256 KiB per rank, each checked element by element."""
    nb.nbody_lib()   # builds the product (and nbody-bench) when missing
    r = subprocess.run([BENCH_EXE, "--gpus", str(P), "--selftest-ranks"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.strip() == f"rank page selftest ok: {P} ranks, 250 all-gathers per rank"


def test_rank_page_a_dying_rank_ends_the_run_quickly():
    """One rank leaves with status 7 while the others wait at a barrier: they notice the failed page, leave with 4, the
    parent reaps all of them and reports the first failure -- well inside the 180 s wait timeout."""
    import time
    nb.nbody_lib()
    t0 = time.time()
    r = subprocess.run([BENCH_EXE, "--gpus", "4", "--selftest-ranks", "--selftest-die", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 7 and time.time() - t0 < 20
    assert "rank 2" in r.stderr and "ended with status 7" in r.stderr and r.stderr.count("leaving (exit 4)") == 3
    assert "selftest ok" not in r.stdout


def test_rank_page_a_hung_rank_is_ended_by_the_parents_budget():
    """--budget-s in the C harness: one rank never reaches the next barrier (a collective that never completes) while the page's
    own wait timeout is far away; the parent -- which only waits and reaps -- ends exactly its children when the attempt has
    used up its share, says so, and leaves non-zero: seconds, not the 60 s wait timeout."""
    import time
    nb.nbody_lib()
    t0 = time.time()
    r = subprocess.run([BENCH_EXE, "--gpus", "3", "--selftest-ranks", "--selftest-hang", "1", "--budget-s", "4", "--wait-timeout", "60"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 4 and 2.0 < time.time() - t0 < 15.0, (r.returncode, r.stderr)
    assert "outlived its 3 s share of the budget; ending its 3 rank(s)" in r.stderr and "selftest ok" not in r.stdout


def test_nbody_bench_cpu_best_column_is_extra_and_labelled():
    """nbody-bench --cpu-best (SURVEY.md 8d's informational row in the C harness): one more column, named CPU*, from the
    fastest CPU variant this host runs (said on stderr, with the reminder that it is not the reference's bits); without the
    flag the table has exactly the reference's columns plus ours, as before."""
    nb.nbody_lib()
    env = dict(os.environ, OMP_NUM_THREADS="2")
    plain = subprocess.run([BENCH_EXE, "--cpu", "--n", "1200", "--steps", "3"], env=env, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.splitlines()[0].split() == ["N", "CPU", "CPU", "int/s"] and "cpu-best" not in plain.stderr
    r = subprocess.run([BENCH_EXE, "--cpu", "--cpu-best", "--n", "1200", "--steps", "3"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    head, row = [l.split() for l in r.stdout.splitlines()[:2]]
    assert head == ["N", "CPU", "CPU*", "CPU", "int/s", "CPU*", "int/s"] and row[0] == "1200" and len(row) == 5
    assert float(row[3]) > 0 and float(row[4]) > 0
    names = [n for n, ok, _ in nb.cpu_variants() if ok]
    assert "informational: not the reference's bits" in r.stderr and (any(f"column = {n} " in r.stderr for n in names) or not names)


def test_nbody_bench_rejects_a_captured_graph_over_the_host_transport():
    nb.nbody_lib()
    r = subprocess.run([BENCH_EXE, "--gpus", "2", "--transport", "shm", "--modes", "plain,graph"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "graph needs --transport rccl" in r.stderr


def test_nbody_bench_walks_rccl_ipc_shm_in_fresh_ranks_and_keeps_the_users_timeout():
    """nbody-bench --gpus P --transport auto = rccl -> ipc -> shm, every attempt in freshly forked ranks.
    Without a GPU every attempt's ranks leave with status 2 (no device), which is enough to see the chain: three attempts, two
    transport_fallback lines naming bring_up_failed, the last attempt's status as the exit code -- and an explicit transport
    makes one attempt only.  A NB_HIP_COMM_TIMEOUT_S the user exported is neither overwritten nor unset."""
    nb.nbody_lib()
    env = dict(os.environ, NB_HIP_COMM_TIMEOUT_S="33")
    r = subprocess.run([BENCH_EXE, "--gpus", "2", "--n", "4096", "--steps", "2"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.stdout, r.stderr)
    marks = [l for l in r.stdout.splitlines() if l.startswith("# transport_fallback")]
    assert [m.split("(")[0].strip() for m in marks] == ["# transport_fallback rccl -> ipc", "# transport_fallback ipc -> shm"]
    assert all("bring_up_failed, status 2" in m for m in marks)
    for name, need in (("rccl", "needs 2 (one per rank)"), ("ipc", "needs 1"), ("shm", "needs 1")):
        assert f"--transport {name} {need}" in r.stderr
    assert "verification_failed" not in r.stdout + r.stderr
    r = subprocess.run([BENCH_EXE, "--gpus", "2", "--n", "4096", "--transport", "shm"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "transport_fallback" not in r.stdout + r.stderr and r.stderr.count("--transport shm needs 1") == 2
    src = open(os.path.join(ROOT, "nbody_amd", "csrc", "bench_main.c")).read()
    assert 'if (!timeout_is_the_users) unsetenv("NB_HIP_COMM_TIMEOUT_S")' in src and src.count('unsetenv("NB_HIP_COMM_TIMEOUT_S")') == 1
    # a budget too small for any attempt still ends with a line that says so, and a non-zero status
    r = subprocess.run([BENCH_EXE, "--gpus", "2", "--n", "4096", "--budget-s", "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 4 and "# budget of 8 s used up before the rccl attempt" in r.stdout


# ---- internal C++ helpers with process-global state, pinned without a GPU -----------------------------------

HELPERS_SRC = r'''
#include "pipeline_internal.h"
#include <chrono>
#include <thread>
#include <atomic>
using namespace nbi;
static void nap(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rand") {
        // the caller's stream: srand(123), then three draws -- with two guards alive on two threads in between
        srand(123);
        const int want[3] = {rand(), rand(), rand()};
        srand(123);
        std::atomic<int> stage{0};
        std::thread other([&] {
            RandGuard g;                 // first guard: swaps a private state in
            stage = 1;
            for (int i = 0; i < 50; i++) { (void)rand(); nap(2); }   // "HIP set-up" drawing from the private state
        });
        while (stage.load() == 0) nap(1);
        {
            RandGuard mine;              // second guard on another thread: must not capture the first one's private state
            RandGuard nested;            // and the same thread may nest (comm_create inside SetSimulationData)
            (void)rand();
        }
        other.join();
        const int got[3] = {rand(), rand(), rand()};
        for (int i = 0; i < 3; i++)
            if (got[i] != want[i]) { printf("rand stream disturbed: draw %d is %d, expected %d\n", i, got[i], want[i]); return 1; }
        printf("rand stream intact\n");
        return 0;
    }
    if (mode == "rand_wait") {
        // two "ranks" on two threads, each inside its first-touch guard, meet at a barrier INSIDE the guarded region (the
        // direct exchange's IPC hand-over runs through the caller's all-gather callback there): must not deadlock
        srand(321);
        const int want[2] = {rand(), rand()};
        srand(321);
        std::atomic<int> arrived{0};
        auto rank = [&] {
            RandGuard first_touch;
            (void)rand();
            arrived++;
            for (int i = 0; i < 3000 && arrived.load() < 2; i++) nap(1);   // the "callback": waits for the peer, 3 s at most
            RandGuard nested;
            (void)rand();
        };
        std::thread a(rank), b(rank);
        a.join();
        b.join();
        if (arrived.load() != 2) { printf("a rank never reached the barrier\n"); return 1; }
        const int got[2] = {rand(), rand()};
        if (got[0] != want[0] || got[1] != want[1]) { printf("rand stream disturbed\n"); return 1; }
        printf("ranks met inside their guards; rand stream intact\n");
        return 0;
    }
    if (mode == "watch") {
        // thread A sits in a long bounded wait; thread B's shorter wait must be watched too (and fire)
        setenv("NB_HIP_COMM_TIMEOUT_S", "60", 1);
        std::atomic<int> stage{0};
        std::thread a([&] {
            Watchdog dog("a long wait on thread A", 0, 2);
            Watchdog inner("nested on thread A: the outer deadline stands", 0, 2);
            stage = 1;
            nap(8000);
        });
        while (stage.load() == 0) nap(1);
        setenv("NB_HIP_COMM_TIMEOUT_S", "1", 1);
        {
            Watchdog quick("a short wait on thread B that completes", 1, 2);
            nap(100);
        }
        printf("first wait on B returned\n");
        fflush(stdout);
        Watchdog dog("the wait on thread B that never completes", 1, 2);
        nap(6000);
        printf("NOT REACHED\n");
        a.join();
        return 0;
    }
    return 2;
}
'''


@pytest.fixture(scope="module")
def helpers_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("helpers")
    (d / "t.cpp").write_text(HELPERS_SRC)
    exe = str(d / "t")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "nbody_amd", "csrc"), str(d / "t.cpp"), "-o", exe, "-L" + nb.LIB_DIR, "-lnbody_hip",
                    "-Wl,-rpath," + nb.LIB_DIR, "-lpthread"], check=True, capture_output=True, timeout=300)
    return exe


def test_rand_guards_on_two_threads_leave_the_callers_stream_alone(helpers_exe):
    """RandGuard (pipeline_internal.h) swaps libc's process-global random state around the first device set-up; two guards
    alive at once on two threads must not hand each other's private state back to the caller: the guard is counted
    process-wide (first in saves the caller's state, last out restores it).  The reference harness draws its universes from
    rand() between GPU calls (src/bench.c:42,53)."""
    r = subprocess.run([helpers_exe, "rand"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "rand stream intact" in r.stdout, (r.stdout, r.stderr)


def test_ranks_on_threads_can_wait_for_each_other_inside_their_rand_guards(helpers_exe):
    """SetSimulationData's first-touch guard spans the caller's all-gather callback (IPC-handle exchange, "ready"
    barrier).  Two ranks driven from two threads of one process must be able to meet there: no lock is held across the
    guarded region, and the caller's rand() stream is still intact afterwards."""
    import time
    t0 = time.time()
    r = subprocess.run([helpers_exe, "rand_wait"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ranks met inside their guards" in r.stdout and time.time() - t0 < 2.5, (r.stdout, r.stderr)


def test_watchdog_watches_waits_on_every_thread(helpers_exe):
    """One watcher thread, one entry per waiting thread: while thread A sits in a wait with a 60 s bound, a wait on thread B
    with a 1 s bound that completes is disarmed without tripping, and one that never completes ends the process with B's
    diagnostic and exit code 3 -- the single-slot watcher of round 4 left that second wait unbounded."""
    import time
    t0 = time.time()
    r = subprocess.run([helpers_exe, "watch"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and time.time() - t0 < 5.0, (r.returncode, r.stdout, r.stderr)
    assert "first wait on B returned" in r.stdout and "NOT REACHED" not in r.stdout
    assert "rank 1 of 2: the wait on thread B that never completes did not complete within 1 s" in r.stderr
