"""What the groups suite could not provoke, without a GPU.

1. The union-find of nbody_amd/csrc/group_common.h held to its argument over schedules: tests/group_schedule.c compiles
   nb_group_find and nb_group_unite as they stand in the header, runs them on logical threads under a scheduler that picks every
   interleaving and every stale value a load may return, and checks the invariants of the argument after every operation, per call
   and at the end.  Every tiny case walked to exhaustion in both thread shapes, seeded random schedules on 32 to 64 nodes and
   8 threads, and the teeth: the same program built over copies of the two functions with one defect planted in each must report
   a failure on the case named beside the defect.
2. The premise of the mask-edge cases (tests/group_edge_cases.py) that tests/test_gpu_group_edges.py runs on the device: every
   planted particle carries a link whose loss changes a label, as a source and as a receiver; the model is the plain double loop
   and the host path is the model on every case.
3. The host path at 16 threads on the two worlds where every hook meets in one tree, five calls each."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import group_edge_cases as ge
import group_ref as gr
import nbody_amd as nb

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TESTS = os.path.join(ROOT, "tests")
COMMON = os.path.join(ROOT, "nbody_amd", "csrc", "group_common.h")
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))

# (shape, loads, case): the device shape costs a load more per source, so its walks are the longer ones.  Left out because they
# do not finish in the time a suite has (counted once, by hand): star_4 in the device shape (2.6e7 schedules with fresh loads), and
# in the device shape with stale loads crossed_pairs_4 (1.3e7) and triangle_3 (3.9e6; it runs with fresh loads)
TINY = ("two_hooks_3", "shared_source_3", "two_components_4", "chain_4", "triangle_3", "crossed_pairs_4", "star_4")
EXHAUSTIVE = ([("host", loads, case) for loads in ("stale", "fresh") for case in TINY]
              + [("device", "stale", case) for case in TINY[:4]]
              + [("device", "fresh", case) for case in TINY[:6]])

# (kind, nodes, runs) for each shape, kind of load and seed: about 16 s of one core in all
RANDOM = (("chain", 32, 4000), ("chain", 64, 2000), ("two_chains", 48, 4000), ("clique", 32, 1000), ("clique", 64, 200))
SEEDS = (1, 2)

FIND_TO_UNITE = re.compile(r"^NB_PAIR_HD uint32_t nb_group_find\(.*?^}\n.*?^NB_PAIR_HD uint32_t nb_group_unite\(.*?^}\n", re.M | re.S)

# defect -> (the text of group_common.h it replaces, what it puts there, the committed case that catches it, what the program says)
DEFECTS = {
    # a failed compare-and-swap gives up instead of going on with the returned value: the hook is lost
    "failed_cas_gives_up": ("if (old == hi) return lo;", "return lo;",
                            ("host", "fresh", "exhaustive", "two_hooks_3"), "does not end at the smallest index of its component"),
    # the hook by an atomic minimum: taken whether or not hi is still a root, so hi's old parent loses its only way down
    "hook_by_min": ("const uint32_t old = NB_GROUP_CAS(parent + hi, hi, lo);", "NB_GROUP_MIN(parent + hi, lo);\n        const uint32_t old = hi;",
                    ("host", "fresh", "exhaustive", "two_hooks_3"), "does not end at the smallest index of its component"),
    # the hook by a plain store
    "hook_by_store": ("const uint32_t old = NB_GROUP_CAS(parent + hi, hi, lo);", "NB_GROUP_STORE(parent + hi, lo);\n        const uint32_t old = hi;",
                      ("host", "fresh", "exhaustive", "two_hooks_3"), None),
    # the larger root stored into the smaller
    "larger_into_smaller": ("const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;", "const uint32_t hi = a > b ? b : a, lo = a > b ? a : b;",
                            ("host", "fresh", "exhaustive", "two_hooks_3"), "a stored value exceeds the word's previous value"),
    # compression as a load followed by a store: it can raise a word another thread lowered in between.  That takes a tree three
    # links deep and two finds racing through it, more than a tiny case holds: the first seeded chain of RANDOM catches it
    "compress_by_store": ("if (g < p) NB_GROUP_MIN(parent + x, g);", "if (g < p) NB_GROUP_STORE(parent + x, g);",
                          ("host", "fresh", "random", "chain", 32, 8, 1, 4000), "a stored value exceeds the word's previous value"),
}
# A failed compare-and-swap followed by a re-read of memory in place of the returned value: see the test of its own below
REREAD = ("a = old;", "a = NB_GROUP_LOAD(parent + hi);")


def compile_checker(out_dir, variant=None):
    cc = os.environ.get("CC", "cc")
    exe = str(out_dir / ("group_schedule" + ("_" + variant if variant else "")))
    cmd = [cc, "-O2", "-std=gnu11", "-Wall", f"-I{ROOT}/include", f"-I{ROOT}/nbody_amd/csrc", f"-I{TESTS}",
           os.path.join(TESTS, "group_schedule.c"), "-o", exe]
    if variant:
        cmd += [f'-DGROUP_VARIANT_HEADER="{out_dir / (variant + ".h")}"']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def planted(out_dir, name, old, new):
    """The two functions of group_common.h, copied under other names with `old` replaced by `new`, exactly once."""
    text = open(COMMON).read()
    m = FIND_TO_UNITE.search(text)
    assert m, "nb_group_find and nb_group_unite are no longer where the copy is cut"
    body = m.group(0)
    assert body.count("nb_group_find(") == 3 and body.count("nb_group_unite(") == 1, body
    if old is not None:
        assert body.count(old) == 1, (name, "the substitution no longer applies", old)
        body = body.replace(old, new)
        assert new in body and old not in body.replace(new, ""), name
    body = body.replace("nb_group_find(", "variant_find(").replace("nb_group_unite(", "variant_unite(")
    (out_dir / (name + ".h")).write_text(body)
    return compile_checker(out_dir, variant=name)


def run(exe, args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout.strip()


def run_all(exe, jobs):
    with ThreadPoolExecutor(WORKERS) as pool:
        return list(pool.map(lambda args: run(exe, args), jobs))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return compile_checker(tmp_path_factory.mktemp("group_schedule"))


def test_every_tiny_case_is_walked_to_exhaustion_in_both_thread_shapes(checker):
    jobs = [(shape, loads, "exhaustive", case) for shape, loads, case in EXHAUSTIVE]
    total = no_longer_roots = 0
    for args, (rc, out) in zip(jobs, run_all(checker, jobs)):
        print("[group schedule]", out)
        assert rc == 0 and out.startswith("OK ") and ", exhausted," in out, (args, rc, out)          # by exhaustion, not by a cut
        total += int(re.search(r": (\d+) schedules", out).group(1))
        no_longer_roots += int(re.search(r"(\d+) returns of unite no longer a root", out).group(1))
    print(f"[group schedule] {total} schedules in {len(jobs)} exhaustive walks")
    # what unite returns is a node of the joined tree, not above either argument -- and not always a root by the time it returns:
    # the sentence above nb_group_unite says the former, and no caller needs the latter
    assert no_longer_roots > 0
    assert {(s, c) for s, _, c in EXHAUSTIVE} >= {(s, c) for s in ("host", "device") for c in TINY[:5]}
    # a walk that is cut says so: the check above can fail
    rc, out = run(checker, ("host", "stale", "exhaustive", "chain_4", 1000))
    assert rc == 2 and out.startswith("CUT ") and "not exhausted" in out, (rc, out)


def test_seeded_random_schedules_on_32_to_64_nodes_and_8_threads(checker):
    jobs = [(shape, loads, "random", kind, nodes, 8, seed, runs)
            for kind, nodes, runs in RANDOM for shape in ("host", "device") for loads in ("stale", "fresh") for seed in SEEDS]
    total = 0
    for args, (rc, out) in zip(jobs, run_all(checker, jobs)):
        print("[group schedule]", out)
        assert rc == 0 and out.startswith("OK "), (args, rc, out)
        total += int(re.search(r": (\d+) schedules", out).group(1))
    print(f"[group schedule] {total} random schedules in {len(jobs)} runs")


def test_a_copy_without_a_defect_passes_so_a_failure_is_the_defects(tmp_path):
    exe = planted(tmp_path, "control", None, None)
    jobs = sorted({d[2] for d in DEFECTS.values()}) + [("device", "stale", "exhaustive", "shared_source_3"), ("host", "stale", "random", "clique", 32, 8, 1, 200)]
    for args, (rc, out) in zip(jobs, run_all(exe, jobs)):
        assert rc == 0 and out.startswith("OK "), (args, rc, out)


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_a_planted_defect_is_reported_by_its_case(name, tmp_path):
    old, new, args, says = DEFECTS[name]
    exe = planted(tmp_path, name, old, new)
    rc, out = run(exe, args)
    print(f"[group schedule] {name}: {out}")
    assert rc == 1 and out.startswith("FAIL "), (name, rc, out)
    if says:
        assert says in out, (name, out)


def test_a_re_read_after_a_failed_compare_and_swap_ends_only_if_loads_are_fresh(tmp_path):
    """Argument 3 goes on with the value the atomic returned, "never with a re-read".  With loads that see the memory the re-read
    is as right as the returned value: every exhaustive case and the random worlds pass.  With stale loads (argument 4 in its
    strongest reading) the re-read may return hi itself for ever, and the loop never ends: the returned value is what bounds
    unite, not a matter of taste.  Both are asserted, so the defect is not among the required ones of DEFECTS."""
    exe = planted(tmp_path, "reread", *REREAD)
    jobs = [("host", "fresh", "exhaustive", case) for case in TINY[:6]] + [("device", "fresh", "exhaustive", case) for case in TINY[:4]]
    jobs += [(shape, "fresh", "random", kind, 32, 8, 1, 500) for shape in ("host", "device") for kind in ("chain", "clique", "two_chains")]
    for args, (rc, out) in zip(jobs, run_all(exe, jobs)):
        assert rc == 0 and out.startswith("OK "), (args, rc, out)
    rc, out = run(exe, ("host", "stale", "exhaustive", "two_hooks_3"))
    print(f"[group schedule] reread: {out}")
    assert rc == 1 and out.startswith("FAIL ") and "does not terminate" in out, (rc, out)


# ---- the premise of the mask-edge cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ge.MASS_LENS)
def test_every_planted_particle_of_the_edge_cases_carries_a_bridge_as_source_and_as_receiver(m):
    """From the model alone: 1 < n_groups < hi - lo, and for every planted index s the labels change when the pairs with s as
    their source are withheld, and when those with s as their receiver are.  Two exceptions follow from the statement, not from
    the world: lo is the receiver of no pair and hi - 1 the source of none (j < i); and under mass_len 519 the massless class is
    one particle, a range in which nothing can link -- that case is held to its one singleton."""
    for members in gr.MASKS:
        lo, hi = gr.span(members, ge.N, m)
        for length in ge.LENGTHS:
            a, planted = ge.edge_world(ge.N, m, members, length)
            assert int(np.count_nonzero(a[:, 6] > 0)) == m and np.all(a[:m, 6] > 0)
            want = gr.model(a, m, members, length)
            assert gr.same(want, gr.double_loop(a, m, members, length)), (m, members, length, "the model against the double loop")
            w = nb.World(a)
            assert w.particles().tobytes() == a.tobytes()
            got, k = w.groups(length, gr.NAMES[members], return_count=True)
            w.close()
            assert gr.same(got, want) and k == gr.count(want), (m, members, length, "the host path against the model")
            if hi - lo == 1:
                assert (m, members) == (519, gr.MASSLESS) and k == 1 and planted == []
                continue
            assert 1 < k < hi - lo, (m, members, length, k)
            assert {lo, lo + 1, hi - 2, hi - 1} <= set(planted) and all(lo <= s < hi for s in planted)
            assert {i for e in ge.edges_of(lo, hi) for i in (e - 1, e)} <= set(planted)
            for s in planted:
                if s < hi - 1:
                    assert not gr.same(ge.withheld(a, m, members, length, s, True), want), (m, members, length, s, "as a source")
                if s > lo:
                    assert not gr.same(ge.withheld(a, m, members, length, s, False), want), (m, members, length, s, "as a receiver")


def test_the_edge_cases_stand_on_before_and_behind_every_edge_of_the_walk():
    assert len(ge.CASES) == 22 * 3 * 2 and ge.N == 520 and ge.LENGTHS == (gr.length_for(520, b=1.0), gr.length_for(520, b=2.0))
    for k in (8, 32, 64, 128, 256, 384, 512):
        assert {k - 1, k, k + 1} <= set(ge.MASS_LENS), k
    assert ge.edges_of(0, 520) == [8, 32, 128, 256, 512] and ge.edges_of(129, 520) == [136, 160, 256, 512] and ge.edges_of(513, 520) == []
    chains, planted = ge.plan(0, 520)
    assert (0, 1, [0, 326, 327]) in chains and 326 // ge.TILE == 2          # lo with a particle two tiles on
    assert (0, 2, [0, 519, 518, 517]) in chains and (0, 0, [0, 1, 2]) in chains
    # the members of the two ensembles hold the same edges
    assert ge.RAGGED == ((520, 520, 385, 257, 129, 9), (129, 256, 257, 128, 8, 8)) and ge.UNIFORM == (520, (127, 128, 129, 255, 256, 257))


# ---- the host path where every hook meets in one tree ----------------------------------------------------------------------------

HOST_CODE = """
import numpy as np, nbody_amd as nb, group_ref as gr
worlds = [("coincident", gr.coincident(2049, 700), 1.0), ("chain", gr.chain(2049, seed=2050, m=1024)[0], gr.above(1.0))]
for name, a, length in worlds:
    w = nb.World(a); p = w.particles(); m = int(np.count_nonzero(p[:, 6] > 0))
    want = gr.model(p, m, gr.ALL, length)
    assert not want.any(), name          # one group, named by index 0
    for call in range(5):
        got, k = w.groups(length, return_count=True)
        assert gr.same(got, want) and k == 1, (name, call)
    w.close()
print('OK')
"""


def test_the_host_path_at_sixteen_threads_where_every_hook_meets_in_one_tree():
    """The host path goes parallel from 2 000 particles of the mask: 2 049 coincident particles (every pair links) and the
    shuffled chain through both classes, five calls each, every call the bytes of the model."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, TESTS]), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", OMP_NUM_THREADS="16")
    r = subprocess.run([sys.executable, "-c", HOST_CODE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
