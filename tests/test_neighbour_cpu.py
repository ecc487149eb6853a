"""Nearest neighbours and neighbour counts (include/nbody_neighbour.h, include/nbody_batch_neighbour.h) without a GPU: the numpy
model (neighbour_ref.py) against a plain double loop and against itself over any split of the sources, the host path bit for bit
the model, the teeth of the checker against eight defective restatements, the lattice, coincident particles, the radius at a
separation, non-finite state, a poisoned unrequested class, ensembles on the host, every abort with its message, the numpy
helpers, and the static facts of neighbour.hip's two kernel instances."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
import neighbour_ref as nr
from isa_common import compile_isa, functions, kernel_meta
from paircount_ref import world
from test_abi import declared_functions, exported

ROOT = nb.ROOT
HIDDEN = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")
COMBOS = [(r, s) for r in nr.MASKS for s in nr.MASKS]
RADIUS = 1.5


def child(code, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **HIDDEN)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def host(a, r=nr.ALL, s=nr.ALL, radius=None):
    """(result, partitioned particles, mass_len) of a CPU-only World."""
    w = nb.World(a)
    p = w.particles()
    got = w.neighbours(radius, nr.NAMES[r], nr.NAMES[s])
    w.close()
    return got, p, int(np.count_nonzero(p[:, 6] > 0))


def full(result):
    return tuple(a for a in result if a is not None)


# ---- the model itself ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (3, 0), (7, 0), (23, 23), (40, 17)])
def test_the_model_is_a_plain_double_loop_and_any_split_of_the_sources_merges_to_it(n, m):
    a = world(n, m, seed=50 + n, spread=3.0)
    if n >= 23:
        a[3, 0:2] = a[20, 0:2]          # two distinct particles at one place: candidates of one another with q = +0
        a[5, 0], a[9, 1] = np.nan, np.inf
    for r, s in COMBOS:
        for radius in (None, 0.0, 2.0):
            want = full(nr.double_loop(a, m, r, s, radius))
            assert nr.same(full(nr.model(a, m, r, s, radius)), want), (r, s, radius)
            for chunk in (1, 5, 64):
                assert nr.same(full(nr.model(a, m, r, s, radius, chunk=chunk)), want), (r, s, radius, chunk)


def test_the_key_orders_like_the_rule():
    """bits(q) of a q >= +0 order like q, +inf above every finite one and every NaN above +inf; the low word breaks ties."""
    q = np.array([0.0, 1e-45, 1e-38, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), 3e38, np.inf], dtype=np.float32)
    bits = q.view(np.uint32).astype(np.uint64)
    assert np.all(np.diff(bits.astype(np.int64)) > 0) and bits[-1] == nr.INF_BITS
    for nan in (np.float32(np.nan), -np.float32(np.nan)):
        assert np.array([nan], dtype=np.float32).view(np.uint32)[0] > nr.INF_BITS
    key = lambda v, j: (int(np.float32(v).view(np.uint32)) << 32) | j
    assert key(1.0, 7) < key(1.0, 8) < key(np.nextafter(np.float32(1), np.float32(2)), 0) < int(nr.KEY_NONE)
    assert int(nr.KEY_NONE) & 0xFFFFFFFF == nr.NONE == nb.NB_NEIGH_NONE


# ---- the host path is the model, bit for bit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 64, 129, 257, 1000])
def test_host_path_is_bitwise_the_model(n):
    for m in nr.masses(n):
        w = nb.World(world(n, m, seed=n))
        p = w.particles()
        assert int(np.count_nonzero(p[:, 6] > 0)) == m
        for r, s in COMBOS:
            want = nr.model(p, m, r, s, RADIUS)
            got = w.neighbours(RADIUS, nr.NAMES[r], nr.NAMES[s])
            assert [a.shape for a in got] == [(n,)] * 3 and [a.dtype for a in got] == [np.float32, np.uint32, np.uint32]
            assert nr.same(got, want), (n, m, r, s)
            bare = w.neighbours(None, nr.NAMES[r], nr.NAMES[s])
            assert len(bare) == 2 and nr.same(bare, want[:2]), (n, m, r, s, "without a radius")
            r0, r1 = nr.span(r, n, m)
            idle = np.ones(n, dtype=bool)
            idle[r0:r1] = False          # a particle that is no receiver: (+inf, NONE, 0)
            assert np.all(np.isposinf(got[0][idle])) and np.all(got[1][idle] == nr.NONE) and not got[2][idle].any()
        assert nr.same(w.neighbours(), w.neighbours(None, "all", "all"))
        w.close()


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

def test_the_checker_rejects_every_defective_variant():
    """Each defective restatement differs from the host path on a world built to expose it, and the same checker says so."""
    twins = world(64, 30, seed=22)
    twins[40, 0:2] = twins[7, 0:2]          # two distinct particles at one place
    on_radius = world(3, 3, seed=2)
    on_radius[:, 0:2] = [[0.0, 0.0], [3.0, 0.0], [0.0, 40.0]]          # q = 9 = radius^2 exactly
    poisoned = world(64, 30, seed=24)
    poisoned[30:, 0:2] = np.nan          # the massless class, not asked for
    witnesses = {
        "self_included": (world(64, 30, seed=21), nr.ALL, nr.ALL, RADIUS),
        "self_by_position": (twins, nr.ALL, nr.ALL, RADIUS),
        "largest_index": (nr.lattice(6), nr.ALL, nr.ALL, RADIUS),
        "radius_le": (on_radius, nr.ALL, nr.ALL, 3.0),
        "nan_smallest": (nr.nonfinite_worlds()["NaN positions"][0], nr.ALL, nr.ALL, RADIUS),
        "inf_candidate": (nr.nonfinite_worlds()["q overflows"][0], nr.ALL, nr.ALL, RADIUS),
        "source_mask_ignored": (world(64, 30, seed=23), nr.ALL, nr.MASSIVE, RADIUS),
        "unrequested_read": (poisoned, nr.MASSIVE, nr.MASSIVE, RADIUS),
    }
    assert set(witnesses) == set(nr.VARIANTS)
    for variant, (a, r, s, radius) in witnesses.items():
        got, p, m = host(a, r, s, radius)
        assert nr.checker(got, p, m, r, s, radius), variant
        assert not nr.checker(got, p, m, r, s, radius, variant=variant), variant
    q, i, c = host(world(5, 5, seed=1), radius=RADIUS)[0]
    assert nr.same((q, i, c), (q, i, c)) and not nr.same((q, i, c), (q, i)) and not nr.same((q, i, c), (q, i.astype(np.int32), c))
    assert not nr.same((q, i, c), (q, i, c + np.uint32(1)))


# ---- special worlds ------------------------------------------------------------------------------------------------------------

def test_on_a_lattice_the_smallest_index_among_four_equidistant_neighbours_wins():
    side = 9
    (q, index, count), p, m = host(nr.lattice(side), radius=1.25)
    assert m == side * side and nr.checker((q, index, count), p, m, radius=1.25)
    i = np.arange(side * side)
    inner = (i // side > 0) & (i // side < side - 1) & (i % side > 0) & (i % side < side - 1)
    assert np.all(q == 1.0) and np.array_equal(index[inner], (i - side)[inner]) and np.all(count[inner] == 4)
    assert index[0] == 1 and count[0] == 2 and index[side * side - 1] == side * side - 1 - side
    pairs = nb.closest_pairs(q, index, k=4)
    assert pairs == [(0, 1, 1.0), (0, side, 1.0), (1, 2, 1.0), (1, side + 1, 1.0)]          # sorted by (q, i, j); (0, 1) is mutual and appears once
    assert len(nb.closest_pairs(q, index, k=10 ** 6)) == len({(min(a, int(b)), max(a, int(b))) for a, b in enumerate(index)})
    d = nb.neighbour_distance(q)
    assert d.dtype == np.float64 and d.shape == q.shape and np.all(d == 1.0)


def test_coincident_particles_are_candidates_with_q_zero():
    n, m = 70, 25
    a = nr.coincident(n, m)
    for r, s in COMBOS:
        (q, index, count), p, m_ = host(a, r, s, 0.5)
        assert m_ == m and nr.checker((q, index, count), p, m, r, s, 0.5)
        (r0, r1), (s0, s1) = nr.span(r, n, m), nr.span(s, n, m)
        rows = np.arange(r0, r1)
        assert np.all(q[r0:r1] == 0.0) and not np.signbit(q[r0:r1]).any()
        assert np.array_equal(index[r0:r1], np.where(rows == s0, s0 + 1, s0))          # the smallest other index
        assert np.array_equal(count[r0:r1], (s1 - s0) - ((rows >= s0) & (rows < s1)))          # count = candidates
    assert not host(a, radius=0.0)[0][2].any()          # q = +0 is not < 0
    a = world(3, 3, seed=8)
    a[:, 0:2] = [[2.0, 2.0], [2.0, 2.0], [2.0, 3.0]]          # two distinct particles at one place beside a third
    q, index, count = host(a, radius=1.5)[0]
    assert list(q) == [0.0, 0.0, 1.0] and list(index) == [1, 0, 0] and list(count) == [2, 2, 2]


def test_a_radius_below_on_and_above_a_separation():
    a = world(3, 3, seed=2)
    a[:, 0:2] = [[0.0, 0.0], [3.0, 0.0], [0.0, 40.0]]
    three = np.float32(3.0)
    for radius, within in ((np.nextafter(three, np.float32(0)), 0), (three, 0), (np.nextafter(three, np.float32(9)), 1)):
        got, p, m = host(a, radius=float(radius))
        assert nr.checker(got, p, m, radius=float(radius)) and list(got[2]) == [within, within, 0] and list(got[0]) == [9.0, 9.0, 1600.0]
    # a separation whose square is no float32: q = fl(d * d) against the exact (double)d^2, as the pair counts compare
    d = next(v for v in np.array([0.1, 0.3, 0.7, 1.1, 1.3], dtype=np.float32) if np.float64(v * v) < np.float64(v) ** 2)
    a[1, 0] = d
    got, p, m = host(a, radius=float(d))
    assert nr.checker(got, p, m, radius=float(d)) and list(got[2]) == [1, 1, 0]          # q rounded down lies inside the radius


def test_non_finite_state():
    for name, (a, mass_len) in nr.nonfinite_worlds().items():
        bad = ~np.isfinite(a[:, 0]) | ~np.isfinite(a[:, 1])
        for r, s in COMBOS:
            (q, index, count), p, m = host(a, r, s, RADIUS)
            assert m == mass_len and nr.checker((q, index, count), p, m, r, s, RADIUS), (name, r, s)
            assert np.all(np.isposinf(q[bad])) and np.all(index[bad] == nr.NONE) and not count[bad].any(), name          # an own NaN / inf
            assert not np.isin(index[index != nr.NONE], np.nonzero(bad)[0]).any(), name          # never a candidate
        if bad.any():          # a neighbour's NaN changes no other row: the world without those particles answers the same
            keep = np.nonzero(~bad)[0]
            q, index, count = host(a, radius=RADIUS)[0]
            q2, index2, count2 = host(a[keep], radius=RADIUS)[0]
            back = np.where(index2 == nr.NONE, np.uint32(nr.NONE), keep[np.minimum(index2, len(keep) - 1)].astype(np.uint32))
            assert nr.same((q[keep], index[keep], count[keep]), (q2, back, count2)), name
    q, index, count = host(nr.nonfinite_worlds()["q overflows"][0], radius=RADIUS)[0]
    assert np.isposinf(q[0]) and index[0] == nr.NONE and index[3] not in (0, 1, 2)          # a q of +inf is no candidate
    q, index, count = host(nr.nonfinite_worlds()["nobody has a candidate"][0], radius=RADIUS)[0]
    assert np.all(np.isposinf(q)) and np.all(index == nr.NONE) and not count.any()


def test_a_poisoned_unrequested_class_changes_no_bit():
    n, m = 300, 120
    a = world(n, m, seed=9)
    for r, s, lo, hi in ((nr.MASSIVE, nr.MASSIVE, m, n), (nr.MASSLESS, nr.MASSLESS, 0, m)):
        poisoned = a.copy()
        poisoned[lo:hi, 0:6] = np.nan
        clean, dirty = host(a, r, s, RADIUS)[0], host(poisoned, r, s, RADIUS)[0]
        assert nr.same(clean, dirty), (r, s)
        assert not nr.same(host(poisoned, nr.ALL, s, RADIUS)[0], host(a, nr.ALL, s, RADIUS)[0])          # ... and asked for, it is read


# ---- ensembles on the host -----------------------------------------------------------------------------------------------------

def test_a_batch_that_never_stepped_answers_on_the_host_with_the_result_of_each_member_alone():
    members = [world(n, m, seed=40 + n) for n, m in ((1, 1), (2, 0), (333, 0), (257, 257), (700, 350))]
    members[4][5, 0] = np.nan
    wb = nb.WorldBatch.ragged(members)
    for r, s in COMBOS:
        got = wb.neighbours(RADIUS, nr.NAMES[r], nr.NAMES[s])
        assert len(got) == 3 and all(isinstance(a, list) and len(a) == 5 for a in got)
        for b, a in enumerate(members):
            alone, p, m = host(a, r, s, RADIUS)
            assert nr.same(tuple(x[b] for x in got), alone) and nr.checker(alone, p, m, r, s, RADIUS), (r, s, b)
    assert len(wb.neighbours()) == 2
    wb.close()
    states = np.stack([world(250, 100, seed=s) for s in range(3)])
    uniform = nb.WorldBatch(states)
    got = uniform.neighbours(RADIUS)
    assert [a.shape for a in got] == [(3, 250)] * 3 and [a.dtype for a in got] == [np.float32, np.uint32, np.uint32]
    for b in range(3):
        assert nr.same(tuple(x[b] for x in got), nr.model(states[b], 100, radius=RADIUS))
    uniform.close()


def test_cpu_only_worlds_and_batches_never_open_a_device():
    code = ("import os, numpy as np, nbody_amd as nb, neighbour_ref as nr\n"
            "from paircount_ref import world\n"
            "a = world(600, 300, seed=1)\n"
            "w = nb.World(a); w.update_cpu(0.01, 2); got = w.neighbours(1.5); p = w.particles(); w.close()\n"
            "ok = nr.same(got, nr.model(p, 300, radius=1.5))\n"
            "wb = nb.WorldBatch(np.stack([a, a])); gb = wb.neighbours(None, 'massive', 'massless'); wb.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', ok, got[0].shape, len(gb), gb[1].shape)\n")
    r = child(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK True (600,) 2 (2, 600)"


# ---- argument checks -----------------------------------------------------------------------------------------------------------

SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); wb = nb.WorldBatch(np.stack([a, a, a])); L = nb.nbody_lib(); H = nb.hip_lib()\n"
         "q = np.zeros(64, dtype=np.float32); i = np.zeros(64, dtype=np.uint32); c = np.zeros(64, dtype=np.uint32)\n"
         "Q, I, K = q.ctypes.data, i.ctypes.data, c.ctypes.data\n"
         "s = nb.SimPipeline(4, 4); sb = nb.SimBatch(4, [4, 4, 4])\n"
         "def spec(receivers=3, sources=3, radius=1.0):\n"
         "    return C.byref(nb.WorldNeighbourSpec(receivers, sources, radius))\n")
SHARDED = "fn = nb.ALLGATHER_FN(lambda *x: None); ws = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
RECEIVERS = "receivers must be a non-empty set of NB_NEIGH_MASSIVE | NB_NEIGH_MASSLESS"
SOURCES = "sources must be a non-empty set of NB_NEIGH_MASSIVE | NB_NEIGH_MASSLESS"
FINITE, NEGATIVE = "radius must be finite", "radius must not be negative"
ABORTS = [
    # the World layer
    ("world NULL world", "L.GetWorldNeighbours(None, spec(), Q, I, K)", "NULL argument"),
    ("world NULL spec", "L.GetWorldNeighbours(w._h, None, Q, I, K)", "NULL argument"),
    ("world NULL q", "L.GetWorldNeighbours(w._h, spec(), None, I, K)", "NULL argument"),
    ("world NULL index", "L.GetWorldNeighbours(w._h, spec(), Q, None, K)", "NULL argument"),
    ("world receivers 0", "w.neighbours(1.0, receivers=0)", RECEIVERS),
    ("world receivers 4", "w.neighbours(1.0, receivers=4)", RECEIVERS),
    ("world sources 0", "w.neighbours(sources=0)", SOURCES),
    ("world sources 7", "w.neighbours(sources=7)", SOURCES),
    ("world radius NaN", "w.neighbours(float('nan'))", FINITE),
    ("world radius inf", "w.neighbours(float('inf'))", FINITE),
    ("world radius negative", "w.neighbours(-0.5)", NEGATIVE),
    ("sharded world", SHARDED + "L.GetWorldNeighbours(ws, spec(), Q, I, K)", "GetWorldNeighbours of a sharded pipeline needs a collective"),
    # the batch layer
    ("batch NULL batch", "L.GetWorldBatchNeighbours(None, spec(), Q, I, K)", "GetWorldBatchNeighbours: NULL argument"),
    ("batch NULL spec", "L.GetWorldBatchNeighbours(wb._h, None, Q, I, K)", "GetWorldBatchNeighbours: NULL argument"),
    ("batch NULL q", "L.GetWorldBatchNeighbours(wb._h, spec(), None, I, K)", "GetWorldBatchNeighbours: NULL argument"),
    ("batch NULL index", "L.GetWorldBatchNeighbours(wb._h, spec(), Q, None, None)", "GetWorldBatchNeighbours: NULL argument"),
    ("batch receivers 8", "wb.neighbours(receivers=8)", RECEIVERS),
    ("batch sources 0", "wb.neighbours(1.0, sources=0)", SOURCES),
    ("batch radius NaN", "wb.neighbours(float('nan'))", FINITE),
    ("batch radius negative", "wb.neighbours(-1.0)", NEGATIVE),
    # the seam: every check comes before any device touch (no device is visible to these children)
    ("seam NULL pipeline", "H.nb_hip_neighbours(None, 3, 3, 1.0, Q, I, K)", "NULL pipeline"),
    ("seam NULL q", "H.nb_hip_neighbours(s._h, 3, 3, 1.0, None, I, K)", "nb_hip_neighbours: NULL argument"),
    ("seam NULL index", "H.nb_hip_neighbours(s._h, 3, 3, 1.0, Q, None, None)", "nb_hip_neighbours: NULL argument"),
    ("seam receivers 0", "s.neighbours(receivers=0)", RECEIVERS),
    ("seam receivers 5", "s.neighbours(1.0, receivers=5)", RECEIVERS),
    ("seam sources 0", "s.neighbours(sources=0)", SOURCES),
    ("seam sources 4", "s.neighbours(1.0, sources=4)", SOURCES),
    ("seam radius NaN", "s.neighbours(float('nan'))", FINITE),
    ("seam radius -inf", "s.neighbours(float('-inf'))", FINITE),
    ("seam radius negative", "s.neighbours(-1e-30)", NEGATIVE),
    ("seam before set_data", "s.neighbours(1.0)", "nb_hip_neighbours before SetSimulationData"),
    ("seam before set_data, no count", "H.nb_hip_neighbours(s._h, 3, 3, float('nan'), Q, I, None)", "nb_hip_neighbours before SetSimulationData"),
    ("ensemble NULL ensemble", "H.nb_hip_ensemble_neighbours(None, 3, 3, 1.0, Q, I, K)", "NULL ensemble"),
    ("ensemble NULL q", "H.nb_hip_ensemble_neighbours(sb._h, 3, 3, 1.0, None, I, K)", "nb_hip_ensemble_neighbours: NULL argument"),
    ("ensemble NULL index", "H.nb_hip_ensemble_neighbours(sb._h, 3, 3, 1.0, Q, None, K)", "nb_hip_ensemble_neighbours: NULL argument"),
    ("ensemble receivers 0", "sb.neighbours(receivers=0)", RECEIVERS),
    ("ensemble sources 16", "sb.neighbours(sources=16)", SOURCES),
    ("ensemble radius inf", "sb.neighbours(float('inf'))", FINITE),
    ("ensemble radius negative", "sb.neighbours(-2.0)", NEGATIVE),
    ("ensemble before set_data", "sb.neighbours(1.0)", "nb_hip_ensemble_neighbours before nb_hip_batch_set_data"),
    ("ragged ensemble before set_data", "nb.SimBatch.ragged([4, 9], [1, 2]).neighbours()", "nb_hip_ensemble_neighbours before nb_hip_batch_set_data"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_the_radius_is_read_only_when_a_count_is_asked_for():
    r = child(SETUP + "L.GetWorldNeighbours(w._h, spec(radius=float('nan')), Q, I, None)\n"
              "L.GetWorldBatchNeighbours(wb._h, spec(radius=-1.0), Q, I, None)\nprint('SURVIVED', [int(v) for v in i[:4]], [float(v) for v in q[:4]])")
    assert r.returncode == 0 and r.stdout.strip() == "SURVIVED [1, 0, 1, 2] [1.0, 1.0, 1.0, 1.0]", (r.stdout, r.stderr)


def test_python_arguments_raise_before_the_library_is_called():
    w = nb.World(world(8, 8))
    for bad in (dict(receivers="mm"), dict(sources="heavy"), dict(receivers=None), dict(sources=("massive",)), dict(receivers=1.5)):
        with pytest.raises(ValueError):
            w.neighbours(**bad)
    w.close()
    q, index = np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.uint32)
    for bad in ((q.reshape(2, 2), index.reshape(2, 2)), (q, index[:3])):
        with pytest.raises(ValueError):
            nb.closest_pairs(*bad)
    with pytest.raises(ValueError):
        nb.closest_pairs(q, index, k=-1)


# ---- the numpy helpers ---------------------------------------------------------------------------------------------------------

def test_the_helpers_return_the_stated_shapes():
    q = np.array([4.0, 0.25, np.inf, 4.0], dtype=np.float32)
    d = nb.neighbour_distance(q)
    assert d.dtype == np.float64 and list(d) == [2.0, 0.5, np.inf, 2.0]
    assert nb.neighbour_distance(np.stack([q, q])).shape == (2, 4)
    index = np.array([3, 3, nr.NONE, 0], dtype=np.uint32)          # 0 <-> 3 is mutual; 2 has nobody
    assert nb.closest_pairs(q, index, k=5) == [(1, 3, 0.25), (0, 3, 4.0)]
    one = nb.closest_pairs(q, index)
    assert one == [(1, 3, 0.25)] and isinstance(one[0][0], int) and isinstance(one[0][2], float)
    assert nb.closest_pairs(q, index, k=0) == [] and nb.closest_pairs(q[:0], index[:0]) == []
    a = world(200, 80, seed=3)
    a[150, 0:2] = a[20, 0:2] + np.float32(1e-3)          # the closest encounter of the world, planted
    got = host(a)[0]
    assert nb.closest_pairs(*got)[0][:2] == (20, 150)


# ---- sources, headers, exports -------------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_neighbour.h") == ["GetWorldNeighbours"]
    assert declared_functions("nbody_batch_neighbour.h") == ["GetWorldBatchNeighbours"]
    funcs, seam = {"GetWorldNeighbours", "GetWorldBatchNeighbours"}, {"nb_hip_neighbours", "nb_hip_ensemble_neighbours"}
    assert funcs <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert funcs <= have and "nb_cpu_neighbours" not in have, so          # the host path is internal
    assert seam <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and seam <= exported(nb.HIP_SO) and not seam & set(nb.TUNE_API)
    assert "nb_hip_neighbour_span" in nb.TUNE_API and "nb_hip_neighbour_span" in exported(nb.HIP_SO)
    assert "nb_hip_neighbour_span" not in declared_functions("nbody_hip.h")
    assert nb.hip_lib().nb_hip_neighbour_span(0) == 0          # auto unless a test says otherwise; host code only
    assert nb.hip_lib().nb_hip_version() == 400          # no version bump: the new surface is detected by its symbols
    text = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert 'dlsym "nb_hip_neighbours"' in text and 'dlsym "nb_hip_ensemble_neighbours"' in text
    header = open(os.path.join(ROOT, "include", "nbody_neighbour.h")).read()
    assert "NB_NEIGH_MASSIVE = 1, NB_NEIGH_MASSLESS = 2" in header and "#define NB_NEIGH_NONE 0xFFFFFFFFu" in header
    assert (nb.NB_NEIGH_MASSIVE, nb.NB_NEIGH_MASSLESS, nb.NB_NEIGH_ALL) == (nr.MASSIVE, nr.MASSLESS, nr.ALL)
    for word in ("k > 1 nearest neighbours", "periodic boundaries", "radius per member", "traced update"):
        assert word in header, word          # what is not built is said
    for cls in (nb.SimPipeline, nb.World, nb.SimBatch, nb.WorldBatch):
        assert callable(getattr(cls, "neighbours")), cls
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\bneighbour\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\bneighbour_cpu\.c", make, re.M)
    assert re.search(r"^\$\(OUT\)/%\.o:.*\$\(HERE\)neighbour_common\.h", make, re.M) and "-ffp-contract=off" in make
    # the statement is written once: neither path restates q or the rule of a pair
    for source in ("neighbour.hip", "neighbour_cpu.c"):
        body = open(os.path.join(csrc, source)).read()
        assert '#include "neighbour_common.h"' in body and "nb_pair_q(" in body and "nb_neigh_take(" in body and "nb_neigh_range(" in body, source
        assert "dx * dx" not in body, source
    common = open(os.path.join(csrc, "neighbour_common.h")).read()
    assert '#include "paircount_common.h"' in common and "dx * dx" not in common


# ---- static ISA of neighbour.hip -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def neighbour_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("neighbour_isa"), "neighbour.hip")


def test_neighbour_hip_holds_two_kernel_instances_without_scratch_within_the_registers_its_header_states(neighbour_isa):
    source = open(os.path.join(ROOT, "nbody_amd", "csrc", "neighbour.hip")).read()
    stated = {"ILb0E": int(re.search(r"neighbour_kernel<false> at most (\d+) VGPRs", source).group(1)),
              "ILb1E": int(re.search(r"neighbour_kernel<true> at most (\d+)", source).group(1))}
    meta = kernel_meta(neighbour_isa)
    assert len(meta) == 2 and all("neighbour_kernel" in m[0] for m in meta), [m[0] for m in meta]
    assert sorted(tag for tag in stated for m in meta if tag in m[0]) == ["ILb0E", "ILb1E"]          # nearest only, nearest + count
    for name, scratch, sgpr, vgpr in meta:
        bound = next(v for tag, v in stated.items() if tag in name)
        print(f"[neighbour isa] {name}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs (stated: at most {bound})")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgpr <= bound <= 64, (name, vgpr, bound)          # 64: eight waves per SIMD, four workgroups of eight waves per CU
    assert re.findall(r"\.max_flat_workgroup_size:\s+(\d+)", neighbour_isa) == ["512", "512"]
    lds = sorted(int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", neighbour_isa))
    assert lds[-1] == 128 * 8 + 128 * 4 and lds[0] in (128 * 8, 128 * 8 + 128 * 4), lds          # the header's 1.5 KiB


def test_q_is_formed_by_multiplies_and_an_add_never_by_an_fma(neighbour_isa):
    bodies = {name: body for name, body in functions(neighbour_isa).items() if "neighbour_kernel" in name}
    assert len(bodies) == 2
    for name, body in bodies.items():
        ops = [ins.split()[0] for ins in body]
        muls = sum(op.startswith(("v_mul_f32", "v_pk_mul_f32")) for op in ops)
        adds = sum(op.startswith(("v_add_f32", "v_pk_add_f32")) for op in ops)
        subs = sum(op.startswith(("v_sub_f32", "v_subrev_f32", "v_pk_add_f32")) for op in ops)
        print(f"[neighbour isa] {name}: {muls} multiplies, {adds} adds, {subs} subtractions")
        assert muls > 0 and adds > 0 and subs > 0, name
        fused = [ins for ins in body if re.match(r"v_(pk_)?(fma|fmac|mad|mac)\w*_f(16|32|64)", ins)]
        assert not fused, (name, fused)          # q is the kernel's only float arithmetic: any fma would be feeding it
