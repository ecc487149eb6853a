"""Pair-separation counts (include/nbody_paircount.h, include/nbody_batch_paircount.h) without a GPU: the numpy model
(paircount_ref.py) against a plain double loop, the host path bit for bit the model, the row rule at its edges and the float32
thresholds of the device, non-finite state, the teeth of the checker against six defective restatements, ensembles on the host,
every abort with its message, nb.pair_curves on a lattice, and the static facts of paircount.hip's kernel."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
import paircount_ref as pr
from isa_common import compile_isa, functions, kernel_meta
from test_abi import declared_functions, exported

ROOT = nb.ROOT
HIDDEN = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")


def child(code, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **HIDDEN)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def host_counts(a, edges, classes=pr.ALL):
    """(rows, unplaced, partitioned particles, mass_len) of a CPU-only World."""
    w = nb.World(a)
    p = w.particles()
    out, lost = w.pair_counts(edges, pr.names(classes), return_unplaced=True)
    w.close()
    return out, lost, p, int(np.count_nonzero(p[:, 6] > 0))


def checker(got, lost, p, m, edges, classes=pr.ALL, variant=None):
    """Is (got, lost) what the model -- or one of its defective variants -- says, sums to the class totals included?"""
    want, want_lost = pr.model(p, m, edges, classes, variant)
    return pr.same(got, want) and pr.same(lost, want_lost) and pr.sums_to_class_totals(got, lost, p.shape[0], m, classes)


# ---- the model itself ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(0, 0), (1, 1), (2, 1), (7, 0), (23, 23), (40, 17)])
def test_the_model_is_a_plain_double_loop(n, m):
    a = pr.world(n, m, seed=50 + n, spread=3.0)
    if n >= 23:
        a[3, 0:2] = a[20, 0:2]          # two distinct particles at one place: a pair with q = +0
        a[5, 0] = np.nan
    for edges in (pr.log_edges(7, 0.5, 20.0), pr.lin_edges(2, 6.0)):
        e2 = [float(e) * float(e) for e in edges]
        want, lost = np.zeros((len(edges) + 1, 3), dtype=np.uint64), np.zeros(3, dtype=np.uint64)
        for i in range(n):
            for j in range(i + 1, n):
                with np.errstate(all="ignore"):
                    dx, dy = np.float32(a[i, 0] - a[j, 0]), np.float32(a[i, 1] - a[j, 1])
                    q = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
                col = 0 if j < m else 1 if i < m else 2
                if np.isnan(q):
                    lost[col] += 1
                else:
                    want[sum(1 for v in e2 if v <= float(q)), col] += 1
        got, got_lost = pr.model(a, m, edges)
        assert pr.same(got, want) and pr.same(got_lost, lost) and pr.sums_to_class_totals(got, got_lost, n, m, pr.ALL)
        for classes in pr.SUBSETS:
            sub = pr.model(a, m, edges, classes)
            assert pr.same(sub[0], pr.masked(want, lost, classes)[0]) and pr.same(sub[1], pr.masked(want, lost, classes)[1])


def test_the_grid_model_is_the_model():
    a = pr.world(700, 0, seed=3)
    a[11, 0], a[650, 1] = np.nan, np.inf
    sets = pr.edge_sets()
    grid = pr.model_grid(a, pr.masses(700), sets)
    for m in pr.masses(700):
        for k, e in enumerate(sets):
            want = pr.model(a, m, e)
            assert pr.same(grid[m, k][0], want[0]) and pr.same(grid[m, k][1], want[1]), (m, k)


# ---- the host path is the model, bit for bit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", pr.SIZES)
def test_host_path_is_bitwise_the_model(n):
    sets = pr.edge_sets()
    assert sorted({len(e) - 1 for e in sets}) == list(pr.BINS)
    grid = pr.model_grid(pr.world(n, 0, seed=n), pr.masses(n), sets)
    for m in pr.masses(n):
        w = nb.World(pr.world(n, m, seed=n))
        p = w.particles()
        assert int(np.count_nonzero(p[:, 6] > 0)) == m
        for k, e in enumerate(sets):
            want, want_lost = grid[m, k] if n > 65 else pr.model(p, m, e)
            for classes in pr.SUBSETS:
                got, lost = w.pair_counts(e, pr.names(classes), return_unplaced=True)
                assert got.shape == (len(e) + 1, 3) and got.dtype == np.uint64 and lost.shape == (3,)
                assert pr.same(got, pr.masked(want, want_lost, classes)[0]) and not lost.any(), (n, m, k, classes)
                assert pr.sums_to_class_totals(got, lost, n, m, classes), (n, m, k, classes)
        assert pr.same(w.pair_counts(sets[0]), w.pair_counts(sets[0], "mm")) and pr.same(w.pair_counts(sets[0], "all"), w.pair_counts(sets[0], pr.ALL))
        w.close()


# ---- the row rule at its edges --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pr.edge_pairs()))
def test_a_pair_on_below_and_above_an_edge(name):
    a, edges, row = pr.edge_pairs()[name]
    got, lost, p, m = host_counts(a, edges)
    assert m == 2 and got[row, 0] == 1 and got.sum() == 1 and not lost.any(), (name, got[:, 0])
    assert checker(got, lost, p, m, edges)
    if name.startswith("edge"):
        t, where = int(name.split()[1]), name.split()[2]
        q = pr.pair_q(p[0, 0], p[0, 1], p[1, 0], p[1, 1])
        e2 = np.float32(edges[t]) * np.float32(edges[t])
        assert q == {"below": np.nextafter(e2, np.float32(0)), "on": e2, "above": np.nextafter(e2, np.float32(np.inf))}[where]
    if name == "coincident, edges[0] = 0":
        assert got[0, 0] == 0          # q = +0 is not < e2[0] = 0: row 0 is empty


def test_the_star_of_edge_offsets_and_the_sign_symmetry():
    a, m, edges = pr.edge_star()
    got, lost, p, m_ = host_counts(a, edges)
    assert m_ == m and checker(got, lost, p, m, edges)
    flipped = a.copy()
    flipped[:, 0:2] = -flipped[:, 0:2]          # every dx and dy changes sign: no q changes a bit
    assert pr.same(host_counts(flipped, edges)[0], got)


def test_the_float32_thresholds_are_the_float64_rule():
    """q >= c[t] <=> (double)q >= e2[t] for q at c[t] and at its two float32 neighbours, over edges whose square is a float32,
    is not one, underflows float32 and overflows it."""
    table = np.sort(np.array([1e-30, 1e-20, 3e-20, 0.1, 1.0 / 3.0, 0.5, 1.5, np.pi, 7.0, 1e3 + 1.0 / 3.0, 2e19, 3e19], dtype=np.float32))
    for edges in (table, pr.log_edges(254), pr.lin_edges(64), pr.EDGES_EXACT):
        bins = len(edges) - 1
        c = np.zeros(nb.NB_PAIRS_TABLE, dtype=np.float32)
        top = nb.hip_lib().nb_hip_pair_thresholds(edges.ctypes.data, bins, c.ctypes.data)
        assert top & (top - 1) == 0 and bins + 2 <= 2 * top < 2 * (bins + 2) and np.all(np.isnan(c[bins + 1:])) and np.all(c[1:bins + 1] >= c[:bins])
        e2 = pr.edge2(edges)
        exact = 0
        for t in range(bins + 1):
            assert c[t] == pr.threshold(edges[t]), t
            exact += np.float64(c[t]) == e2[t]
            for q in (np.nextafter(c[t], np.float32(0)), c[t], np.nextafter(c[t], np.float32(np.inf))):
                assert (q >= c[t]) == (np.float64(q) >= e2[t]), (t, q)
        if edges is table:
            assert 0 < exact < bins + 1 and np.isinf(c[bins]) and c[0] == np.float32(1e-45)          # both kinds, both ends
        # and the device's search over that table is the rule
        qs = np.concatenate([c[:bins + 1], np.nextafter(c[:bins + 1], np.float32(0)), [0.0, np.inf]]).astype(np.float32)
        for q in qs:
            pos, step = 0, top
            while step:
                pos += step if c[pos + step - 1] <= q else 0
                step //= 2
            assert pos == pr.rows_of(np.array([q]), e2)[0], q


# ---- non-finite state ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pr.nonfinite_worlds()))
def test_non_finite_state(name):
    a, mass_len, edges, classes = pr.nonfinite_worlds()[name]
    got, lost, p, m = host_counts(a, edges, classes)
    assert m == mass_len and checker(got, lost, p, m, edges, classes), name
    n, last = a.shape[0], len(edges)
    if name == "one particle at +inf":
        assert not lost.any() and got[last, 0] >= m - 1 and got[last, 1] >= n - m          # its pairs lie in the last row
    if name == "two at +inf on one axis":
        assert list(lost) == [0, 1, 0]          # inf - inf: the one pair of the two is NaN
    if name == "NaN positions":
        assert list(lost) == [2 * (m - 2) + 1, 2 * (n - m) + (m - 2), n - m - 1]
    if name == "massless rows of NaN, mm only":
        clean = a.copy()
        clean[m:, 0:6] = 0.0
        other, other_lost, _, _ = host_counts(clean, edges, classes)
        assert got.tobytes() == other.tobytes() and not lost.any() and not other_lost.any()
        assert host_counts(a, edges, pr.ALL)[1][2] == pr.pair_total(2, n, m)          # ... and asked for, they are read


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

def test_the_checker_rejects_every_defective_variant():
    """Each defective restatement differs from the host path on a committed case, and the same checker says so."""
    on_edge, edges_exact, _ = pr.edge_pairs()["edge 2 on"]
    fused, fused_m, fused_edges = pr.fused_world()
    v = next(v for v in np.array([0.1, 0.3, 0.7, 1.1, 1.3], dtype=np.float32) if np.float64(v * v) < np.float64(v) ** 2)
    inexact = np.array([v, 3.0, 30.0], dtype=np.float32)          # an edge whose square is not a float32 and rounds down ...
    close = np.zeros((2, 8), dtype=np.float32)
    close[1, 0], close[:, 6] = v, 1.0                               # ... and a pair at that distance: q = fl(v * v) < (double)v^2, row 0
    witnesses = {
        "self_pair": (pr.world(64, 30, seed=21), pr.log_edges(7)),
        "ordered_twice": (pr.world(64, 30, seed=22), pr.log_edges(7)),
        "edge_swapped": (on_edge, edges_exact),
        "e2_float32": (close, inexact),
        "fused": (fused, fused_edges),
        "mt_in_mm": (pr.world(64, 30, seed=23), pr.log_edges(7)),
    }
    assert set(witnesses) == set(pr.VARIANTS)
    for variant, (a, edges) in witnesses.items():
        got, lost, p, m = host_counts(a, edges)
        assert checker(got, lost, p, m, edges), variant
        assert not checker(got, lost, p, m, edges, variant=variant), variant
    dx, dy, e = pr.find_fused_witness()          # the committed pair: contraction moves q across the edge's square
    z = np.float32(0)
    lo, hi = sorted([pr.pair_q(dx, dy, z, z), pr.pair_q(dx, dy, z, z, fused=True)])
    assert np.float64(lo) < np.float64(e) ** 2 <= np.float64(hi)
    zeros = np.zeros((3, 3), dtype=np.uint64)
    assert pr.same(zeros, zeros) and not pr.same(zeros, zeros + np.uint64(1)) and not pr.same(zeros.astype(np.int64), zeros)


# ---- ensembles on the host -----------------------------------------------------------------------------------------------------

def test_a_batch_that_never_stepped_answers_on_the_host_with_the_counts_of_each_member_alone():
    edges = pr.log_edges(9, 0.5, 30.0)
    members = [pr.world(n, m, seed=40 + n) for n, m in ((1, 1), (2, 0), (333, 0), (257, 257), (700, 350))]
    members[4][5, 0] = np.nan
    wb = nb.WorldBatch.ragged(members)
    for classes in pr.SUBSETS:
        got, lost = wb.pair_counts(edges, pr.names(classes), return_unplaced=True)
        assert got.shape == (5, 11, 3) and got.dtype == np.uint64 and lost.shape == (5, 3) and lost.dtype == np.uint64
        for b, a in enumerate(members):
            w = nb.World(a)
            alone, alone_lost = w.pair_counts(edges, pr.names(classes), return_unplaced=True)
            w.close()
            assert pr.same(got[b], alone) and pr.same(lost[b], alone_lost), (classes, b)
    assert list(wb.pair_counts(edges, "all", return_unplaced=True)[1][4]) == [349, 350, 0]
    wb.close()
    states = np.stack([pr.world(250, 100, seed=s) for s in range(3)])
    uniform = nb.WorldBatch(states)
    got = uniform.pair_counts(edges, "all")
    assert got.shape == (3, 11, 3) and list(got.sum(axis=1)[0]) == [pr.pair_total(c, 250, 100) for c in range(3)]
    for b in range(3):
        assert pr.same(got[b], pr.model(states[b], 100, edges)[0])
    uniform.close()


def test_cpu_only_worlds_and_batches_never_open_a_device():
    code = ("import os, numpy as np, nbody_amd as nb, paircount_ref as pr\n"
            "a = pr.world(600, 300, seed=1); e = pr.log_edges(16)\n"
            "w = nb.World(a); w.update_cpu(0.01, 2); r = w.pair_counts(e, 'all'); p = w.particles(); w.close()\n"
            "ok = pr.same(r, pr.model(p, 300, e)[0])\n"
            "wb = nb.WorldBatch(np.stack([a, a])); rb = wb.pair_counts(e, ('mm', 'tt')); wb.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', ok, r.shape, rb.shape, int(rb.sum()))\n")
    r = child(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == f"OK True (18, 3) (2, 18, 3) {4 * (300 * 299 // 2)}"


# ---- argument checks -----------------------------------------------------------------------------------------------------------

SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); wb = nb.WorldBatch(np.stack([a, a, a])); L = nb.nbody_lib(); H = nb.hip_lib()\n"
         "e = np.array([0, 1, 2, 3], dtype=np.float32)\n"
         "out = np.zeros(4096, dtype=np.uint64); big = np.arange(300, dtype=np.float32)\n"
         "s = nb.SimPipeline(4, 4); sb = nb.SimBatch(4, [4, 4, 4])\n"
         "def spec(edges=e, bins=3, classes=1):\n"
         "    return C.byref(nb.WorldPairSpec(edges.ctypes.data if edges is not None else None, bins, classes))\n")
SHARDED = "fn = nb.ALLGATHER_FN(lambda *x: None); ws = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
BINS_MSG, FINITE, NEGATIVE, RISING = "bins must be 1 .. 254", "edges must be finite", "edges must not be negative", "edges must be strictly increasing"
CLASSES_MSG = "classes must be a non-empty set of NB_PAIRS_MM | NB_PAIRS_MT | NB_PAIRS_TT"
ABORTS = [
    # the World layer
    ("world NULL world", "L.GetWorldPairCounts(None, spec(), out.ctypes.data, None)", "NULL argument"),
    ("world NULL spec", "L.GetWorldPairCounts(w._h, None, out.ctypes.data, None)", "NULL argument"),
    ("world NULL edges", "L.GetWorldPairCounts(w._h, spec(edges=None), out.ctypes.data, None)", "NULL argument"),
    ("world NULL out", "L.GetWorldPairCounts(w._h, spec(), None, None)", "NULL argument"),
    ("world bins 0", "L.GetWorldPairCounts(w._h, spec(bins=0), out.ctypes.data, None)", BINS_MSG),
    ("world bins 255", "L.GetWorldPairCounts(w._h, spec(edges=big, bins=255), out.ctypes.data, None)", BINS_MSG),
    ("world edge inf", "e[3] = np.inf; w.pair_counts(e)", FINITE),
    ("world edge NaN", "e[1] = np.nan; w.pair_counts(e)", FINITE),
    ("world edge negative", "e[0] = -0.5; w.pair_counts(e)", NEGATIVE),
    ("world edges equal", "e[2] = e[1]; w.pair_counts(e)", RISING),
    ("world edges falling", "w.pair_counts(e[::-1].copy())", RISING),
    ("world classes 0", "w.pair_counts(e, classes=0)", CLASSES_MSG),
    ("world classes 8", "w.pair_counts(e, classes=8)", CLASSES_MSG),
    ("sharded world", SHARDED + "L.GetWorldPairCounts(ws, spec(), out.ctypes.data, None)", "GetWorldPairCounts of a sharded pipeline needs a collective"),
    # the batch layer
    ("batch NULL batch", "L.GetWorldBatchPairCounts(None, spec(), out.ctypes.data, None)", "NULL argument"),
    ("batch NULL spec", "L.GetWorldBatchPairCounts(wb._h, None, out.ctypes.data, None)", "NULL argument"),
    ("batch NULL edges", "L.GetWorldBatchPairCounts(wb._h, spec(edges=None), out.ctypes.data, None)", "NULL argument"),
    ("batch NULL out", "L.GetWorldBatchPairCounts(wb._h, spec(), None, None)", "NULL argument"),
    ("batch bins 0", "L.GetWorldBatchPairCounts(wb._h, spec(bins=0), out.ctypes.data, None)", BINS_MSG),
    ("batch edge NaN", "e[0] = np.nan; wb.pair_counts(e)", FINITE),
    ("batch edge negative", "e[0] = -1; wb.pair_counts(e)", NEGATIVE),
    ("batch edges equal", "e[2] = e[1]; wb.pair_counts(e)", RISING),
    ("batch classes 0", "wb.pair_counts(e, classes=0)", CLASSES_MSG),
    ("batch classes 15", "wb.pair_counts(e, classes=15)", CLASSES_MSG),
    # the seam: every check comes before any device touch (no device is visible to these children)
    ("seam NULL pipeline", "H.nb_hip_pair_counts(None, e.ctypes.data, 3, 1, out.ctypes.data, None)", "NULL pipeline"),
    ("seam NULL edges", "H.nb_hip_pair_counts(s._h, None, 3, 1, out.ctypes.data, None)", "nb_hip_pair_counts: NULL argument"),
    ("seam NULL out", "H.nb_hip_pair_counts(s._h, e.ctypes.data, 3, 1, None, None)", "nb_hip_pair_counts: NULL argument"),
    ("seam bins 0", "H.nb_hip_pair_counts(s._h, e.ctypes.data, 0, 1, out.ctypes.data, None)", BINS_MSG),
    ("seam bins 255", "H.nb_hip_pair_counts(s._h, big.ctypes.data, 255, 1, out.ctypes.data, None)", BINS_MSG),
    ("seam edge NaN", "e[2] = np.nan; s.pair_counts(e)", FINITE),
    ("seam edge negative", "e[0] = -1; s.pair_counts(e)", NEGATIVE),
    ("seam edges equal", "e[3] = e[2]; s.pair_counts(e)", RISING),
    ("seam classes 0", "s.pair_counts(e, classes=0)", CLASSES_MSG),
    ("seam classes 9", "s.pair_counts(e, classes=9)", CLASSES_MSG),
    ("seam before set_data", "s.pair_counts(e)", "nb_hip_pair_counts before SetSimulationData"),
    ("ensemble NULL ensemble", "H.nb_hip_ensemble_pair_counts(None, e.ctypes.data, 3, 1, out.ctypes.data, None)", "NULL ensemble"),
    ("ensemble NULL edges", "H.nb_hip_ensemble_pair_counts(sb._h, None, 3, 1, out.ctypes.data, None)", "nb_hip_ensemble_pair_counts: NULL argument"),
    ("ensemble NULL out", "H.nb_hip_ensemble_pair_counts(sb._h, e.ctypes.data, 3, 1, None, None)", "nb_hip_ensemble_pair_counts: NULL argument"),
    ("ensemble bins 255", "H.nb_hip_ensemble_pair_counts(sb._h, big.ctypes.data, 255, 1, out.ctypes.data, None)", BINS_MSG),
    ("ensemble edges falling", "sb.pair_counts(e[::-1].copy())", RISING),
    ("ensemble edge inf", "e[3] = np.inf; sb.pair_counts(e)", FINITE),
    ("ensemble classes 16", "sb.pair_counts(e, classes=16)", CLASSES_MSG),
    ("ensemble before set_data", "sb.pair_counts(e)", "nb_hip_ensemble_pair_counts before nb_hip_batch_set_data"),
    ("ragged ensemble before set_data", "nb.SimBatch.ragged([4, 9], [1, 2]).pair_counts(e)", "nb_hip_ensemble_pair_counts before nb_hip_batch_set_data"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_python_arguments_raise_before_the_library_is_called():
    w = nb.World(pr.world(8, 8))
    e = pr.log_edges(4)
    for bad in (dict(edges=[1.0]), dict(edges=e.reshape(1, -1)), dict(edges=e, classes="mx"), dict(edges=e, classes=("mm", "xx")),
                dict(edges=e, classes=()), dict(edges=e, classes=None), dict(edges=e, classes=1.5)):
        with pytest.raises(ValueError):
            w.pair_counts(**bad)
    w.close()


# ---- the numpy helper ----------------------------------------------------------------------------------------------------------

def test_pair_curves_on_a_lattice_whose_shells_can_be_written_down():
    """A 5 x 5 unit lattice: 40 pairs at distance 1, 32 at sqrt 2, 30 at 2, 48 at sqrt 5, 300 in all."""
    a = np.zeros((25, 8), dtype=np.float32)
    a[:, 0], a[:, 1] = np.repeat(np.arange(5), 5), np.tile(np.arange(5), 5)
    a[:, 6], a[:, 7] = 1.0, 0.25
    edges = np.array([0.5, 1.2, 1.5, 2.1, 2.3], dtype=np.float32)
    w = nb.World(a)
    rows = w.pair_counts(edges)
    assert list(rows[:, 0]) == [0, 40, 32, 30, 48, 150] and not rows[:, 1:].any()
    c = nb.pair_curves(rows, edges)
    assert set(c) == {"r_mid", "area", "density", "cumulative"} and c["density"].shape == (4, 3) and c["cumulative"].shape == (5, 3)
    e = edges.astype(np.float64)
    assert np.allclose(c["r_mid"], 0.5 * (e[1:] + e[:-1])) and np.allclose(c["area"], np.pi * (e[1:] ** 2 - e[:-1] ** 2))
    assert np.allclose(c["density"][:, 0], np.array([40, 32, 30, 48]) / c["area"] / 300.0, rtol=1e-15)
    assert np.allclose(c["cumulative"][:, 0], np.array([0, 40, 72, 102, 150]) / 300.0, rtol=1e-15)
    assert np.all(np.isnan(c["density"][:, 1:])) and np.all(np.isnan(c["cumulative"][:, 1:]))          # classes without a pair
    wide = np.array([0.5, 3.0, 6.0], dtype=np.float32)          # nothing beyond the last edge (the diagonal is 5.66)
    assert nb.pair_curves(w.pair_counts(wide), wide)["cumulative"][-1, 0] == 1.0
    w.close()
    both = nb.pair_curves(np.stack([rows, rows]), edges)          # ensembles: leading axes pass through
    assert both["density"].shape == (2, 4, 3) and np.array_equal(both["cumulative"][1, :, 0], c["cumulative"][:, 0])
    with pytest.raises(ValueError):
        nb.pair_curves(np.zeros((5, 3)), edges)
    with pytest.raises(ValueError):
        nb.pair_curves(np.zeros((6, 6)), edges)


# ---- sources, headers, exports -----------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_paircount.h") == ["GetWorldPairCounts"]
    assert declared_functions("nbody_batch_paircount.h") == ["GetWorldBatchPairCounts"]
    funcs, seam = {"GetWorldPairCounts", "GetWorldBatchPairCounts"}, {"nb_hip_pair_counts", "nb_hip_ensemble_pair_counts"}
    assert funcs <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert funcs <= have and "nb_cpu_pair_counts" not in have, so          # the host path is internal
    assert seam <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and seam <= exported(nb.HIP_SO) and not seam & set(nb.TUNE_API)
    assert nb.hip_lib().nb_hip_version() == 400          # no version bump: the new surface is detected by its symbols
    text = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert 'dlsym "nb_hip_pair_counts"' in text and 'dlsym "nb_hip_ensemble_pair_counts"' in text
    header = open(os.path.join(ROOT, "include", "nbody_paircount.h")).read()
    assert re.search(rf"#define NB_PAIRS_MAX_BINS {nb.NB_PAIRS_MAX_BINS}u\b", header)
    assert "NB_PAIRS_MM = 1, NB_PAIRS_MT = 2, NB_PAIRS_TT = 4" in header and (nb.NB_PAIRS_MM, nb.NB_PAIRS_MT, nb.NB_PAIRS_TT) == (pr.MM, pr.MT, pr.TT)
    for word in ("Mass-weighted", "periodic boundaries", "per-member edges"):
        assert word.lower() in header.lower(), word          # what is not built is said
    for cls in (nb.SimPipeline, nb.World, nb.SimBatch, nb.WorldBatch):
        assert callable(getattr(cls, "pair_counts")), cls
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\bpaircount\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\bpaircount_cpu\.c", make, re.M)
    assert re.search(r"^\$\(OUT\)/%\.o:.*\$\(HERE\)paircount_common\.h", make, re.M) and "-ffp-contract=off" in make
    # the statement is written once: neither path restates q
    for source in ("paircount.hip", "paircount_cpu.c"):
        body = open(os.path.join(csrc, source)).read()
        assert '#include "paircount_common.h"' in body and "nb_pair_q(" in body, source
        assert "dx * dx" not in body and "e2[mid]" not in body, source


# ---- static ISA of paircount.hip ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("paircount_isa"), "paircount.hip")


def test_paircount_hip_holds_one_kernel_without_scratch_within_the_registers_its_header_states(pair_isa):
    source = open(os.path.join(ROOT, "nbody_amd", "csrc", "paircount.hip")).read()
    stated = int(re.search(r"pair_count_kernel at most (\d+) VGPRs", source).group(1))
    meta = kernel_meta(pair_isa)
    assert len(meta) == 1 and "pair_count_kernel" in meta[0][0], [m[0] for m in meta]
    for name, scratch, sgpr, vgpr in meta:
        print(f"[paircount isa] {name}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs (stated: at most {stated})")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgpr <= stated <= 72, (name, vgpr, stated)          # 72: seven waves per SIMD, three workgroups of eight waves per CU
    assert re.findall(r"\.max_flat_workgroup_size:\s+(\d+)", pair_isa) == ["512"]


def test_q_is_formed_by_two_multiplies_and_an_add_never_by_an_fma(pair_isa):
    bodies = [body for name, body in functions(pair_isa).items() if "pair_count_kernel" in name]
    assert len(bodies) == 1
    ops = [ins.split()[0] for ins in bodies[0]]
    muls = sum(op.startswith(("v_mul_f32", "v_pk_mul_f32")) for op in ops)
    adds = sum(op.startswith(("v_add_f32", "v_pk_add_f32")) for op in ops)
    subs = sum(op.startswith(("v_sub_f32", "v_subrev_f32", "v_pk_add_f32")) for op in ops)
    print(f"[paircount isa] {muls} multiplies, {adds} adds, {subs} subtractions")
    assert muls > 0 and adds > 0 and subs > 0
    fused = [ins for ins in bodies[0] if re.match(r"v_(pk_)?(fma|fmac|mad|mac)\w*_f(16|32|64)", ins)]
    assert not fused, fused          # q is the kernel's only float arithmetic: any fma would be feeding it
