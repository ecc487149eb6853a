"""Friends-of-friends groups (include/nbody_group.h, include/nbody_batch_group.h) without a GPU: the numpy model (group_ref.py)
against a plain double loop with a depth-first search, the host path bit for bit the model at 1 thread and at 16, the teeth of
the checker against nine defective restatements, the shuffled chain on both sides of the float32 edge, interleaved chains, the
lattice, coincident particles, non-finite state, a poisoned class outside the mask, ensembles on the host, every abort with its
message, the numpy helpers, and the static facts of group.hip's three kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import group_ref as gr
import nbody_amd as nb
from isa_common import compile_isa, functions, kernel_meta
from paircount_ref import find_fused_witness, world
from test_abi import declared_functions, exported

ROOT = nb.ROOT
HIDDEN = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")
SIZES = (1, 2, 3, 17, 127, 128, 129, 255, 256, 257, 300)


def child(code, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **HIDDEN)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)


def host(a, members=gr.ALL, linking_length=1.0, count=False):
    """(labels[, n_groups], partitioned particles, mass_len) of a CPU-only World."""
    w = nb.World(a)
    p = w.particles()
    got = w.groups(linking_length, gr.NAMES[members], return_count=count)
    w.close()
    return got, p, int(np.count_nonzero(p[:, 6] > 0))


# ---- the model itself ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_the_model_is_a_plain_double_loop_and_a_depth_first_search(n):
    for m in (gr.masses(n) if n <= 129 else (0, n // 3, n)):
        a = world(n, m, seed=70 + n, spread=3.0)
        if n >= 17:
            a[3, 0:2] = a[12, 0:2]          # two distinct particles at one place
            a[5, 0], a[9, 1] = np.nan, np.inf
        for members in gr.MASKS:
            for length in ((0.0, gr.length_for(n)) if n > 129 else (0.0, gr.length_for(n, b=0.5), gr.length_for(n), gr.length_for(n, b=3.0))):
                want = gr.double_loop(a, m, members, length)
                assert gr.same(gr.model(a, m, members, length), want), (n, m, members, length)


# ---- the host path is the model, bit for bit, whatever the thread count --------------------------------------------------------

HOST_CODE = """
import numpy as np, nbody_amd as nb, group_ref as gr
from paircount_ref import world
checked = 0
for n in %r:
    for m in gr.masses(n):
        w = nb.World(world(n, m, seed=n, spread=3.0)); p = w.particles()
        assert int(np.count_nonzero(p[:, 6] > 0)) == m
        for members in gr.MASKS:
            for b in (0.5, 1.0, 2.0):
                length = gr.length_for(n, b=b)
                got, k = w.groups(length, gr.NAMES[members], return_count=True)
                want = gr.model(p, m, members, length)
                assert got.shape == (n,) and gr.same(got, want), (n, m, members, length)
                assert k == gr.count(want), (n, m, members, length)
                lo, hi = gr.span(members, n, m)
                idle = np.ones(n, dtype=bool); idle[lo:hi] = False
                assert np.all(got[idle] == gr.NONE) and np.all(got[lo:hi] <= np.arange(lo, hi))
                checked += 1
        w.close()
sizes = {}
for n in (2049, 6000):
    a = nb.make_galaxies(n, 2, seed=n, own_rng=True)
    w = nb.World(a); p = w.particles(); m = int(np.count_nonzero(p[:, 6] > 0))
    lo, hi = p[:, 0:2].min(axis=0), p[:, 0:2].max(axis=0)
    length = nb.linking_length_for(n, float(np.prod(hi - lo)), 0.2)
    for members in gr.MASKS:
        got = w.groups(length, gr.NAMES[members])
        assert gr.same(got, gr.model(p, m, members, length)), (n, members)
    sizes[n] = int(nb.group_table(w.groups(length))[1][0])
    w.close()
print('OK', checked, sorted(sizes), all(v > 1 for v in sizes.values()))
"""


@pytest.mark.parametrize("threads", [1, 16])
def test_host_path_is_bitwise_the_model_at_one_thread_and_at_sixteen(threads):
    r = child(HOST_CODE % (SIZES,), OMP_NUM_THREADS=str(threads))
    assert r.returncode == 0, r.stderr
    combos = sum(len(gr.masses(n)) for n in SIZES) * 9
    assert r.stdout.strip() == f"OK {combos} [2049, 6000] True", r.stdout


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

def test_the_checker_rejects_every_defective_variant():
    """Each defective restatement differs from the host path on a world built to expose it, and the same checker says so."""
    on_length = gr.blank(3)
    on_length[:, 0:2] = [[0.0, 0.0], [3.0, 0.0], [0.0, 40.0]]          # q = 9 = linking_length^2 exactly
    twins = world(64, 30, seed=22)
    twins[40, 0:2] = twins[7, 0:2]          # two distinct particles at one place, far from the rest
    twins[40, 0] = twins[7, 0] = np.float32(500.0)
    bridge = gr.blank(3, 2)
    bridge[:, 0] = [0.0, 2.0, 1.0]          # a massless particle between two massive ones
    dx, dy, e = find_fused_witness()
    fused = gr.blank(2)
    fused[1, 0:2] = (dx, dy)
    v = next(v for v in np.array([0.1, 0.3, 0.7, 1.1, 1.3], dtype=np.float32) if np.float64(v * v) < np.float64(v) ** 2)
    inexact = gr.blank(2)
    inexact[1, 0] = v          # q = fl(v * v) lies below the exact v^2: linked under the float64 rule, not under fl(l * l)
    nan = world(40, 20, seed=25, spread=3.0)
    nan[11, 0] = np.nan
    witnesses = {
        "le": (on_length, gr.ALL, 3.0),
        "largest_index": (gr.lattice(4), gr.ALL, 1.5),
        "one_sweep": (gr.chain(17, seed=3)[0], gr.ALL, 1.5),
        "mask_bridges": (bridge, gr.MASSIVE, 1.5),
        "fused": (fused, gr.ALL, float(e)),
        "l2_float32": (inexact, gr.ALL, float(v)),
        "coincident_unlinked": (twins, gr.ALL, 0.5),
        "nan_links": (nan, gr.ALL, 0.25),
    }
    assert set(witnesses) | {"global_labels"} == set(gr.VARIANTS)
    for variant, (a, members, length) in witnesses.items():
        got, p, m = host(a, members, length)
        assert gr.checker(got, p, m, members, length), variant
        assert not gr.checker(got, p, m, members, length, variant=variant), variant
    # labels of an ensemble count within the member
    parts = [gr.lattice(3), gr.lattice(4)]
    wb = nb.WorldBatch.ragged(parts)
    got = wb.groups(1.5)
    wb.close()
    assert all(gr.same(g, w) for g, w in zip(got, gr.ensemble(parts, [9, 16], gr.ALL, 1.5)))
    assert not all(gr.same(g, w) for g, w in zip(got, gr.ensemble(parts, [9, 16], gr.ALL, 1.5, variant="global_labels")))
    lab = host(world(5, 5, seed=1), linking_length=2.0)[0]
    assert gr.same(lab, lab) and not gr.same(lab, lab[:4]) and not gr.same(lab, lab.astype(np.int32)) and not gr.same(lab, lab + np.uint32(1))


# ---- special worlds ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [300, 2049])
def test_the_shuffled_chain_on_both_sides_of_the_float32_edge(n):
    """x = k in a shuffled index order: the link graph has diameter n - 1 and every link hops between arbitrary indices.  At a
    linking length of exactly 1, q = 1 is not < 1: n singletons.  One float32 above, one group labelled 0."""
    a, k = gr.chain(n, seed=n)
    (lab, groups), p, m = host(a, linking_length=1.0, count=True)
    assert np.array_equal(lab, np.arange(n, dtype=np.uint32)) and groups == n and gr.checker(lab, p, m, gr.ALL, 1.0)
    (lab, groups), p, m = host(a, linking_length=gr.above(1.0), count=True)
    assert not lab.any() and lab.dtype == np.uint32 and groups == 1 and gr.checker(lab, p, m, gr.ALL, gr.above(1.0))


def test_two_interleaved_chains_are_two_groups_named_by_their_smallest_indices():
    n = 301
    a, k = gr.two_chains(n, seed=4)
    length = gr.above(2.0)
    (lab, groups), p, m = host(a, linking_length=length, count=True)
    even, odd = np.nonzero(k % 2 == 0)[0], np.nonzero(k % 2 == 1)[0]
    assert groups == 2 and np.all(lab[even] == even.min()) and np.all(lab[odd] == odd.min()) and min(even.min(), odd.min()) == 0
    assert sorted(set(lab)) == sorted({even.min(), odd.min()}) and gr.checker(lab, p, m, gr.ALL, length)
    assert host(a, linking_length=2.0, count=True)[0][1] == n          # q = 4 is not < 4


def test_the_lattice_below_on_and_above_the_spacing_and_above_the_diagonal():
    side = 9
    a = gr.lattice(side)
    n = side * side
    for length, groups in ((0.999, n), (1.0, n), (gr.above(1.0), 1), (1.5, 1)):
        (lab, k), p, m = host(a, linking_length=length, count=True)
        assert k == groups and gr.checker(lab, p, m, gr.ALL, length), length
        assert np.array_equal(lab, np.arange(n) if groups == n else np.zeros(n)), length
    sparse = gr.lattice(side, spacing=2.0)
    sparse = sparse[(np.arange(n) // side + np.arange(n) % side) % 2 == 0]          # a checkerboard: nearest others on the diagonal, sqrt(8) away
    for length, one in ((2.0, False), (float(np.float32(np.sqrt(8.0))), False), (2.83, True)):          # fl(sqrt 8)^2 < 8; 2.83^2 > 8
        (lab, k), p, m = host(sparse, linking_length=length, count=True)
        assert (k == 1) == one and (one or k == len(sparse)) and gr.checker(lab, p, m, gr.ALL, length), length


def test_all_coincident_is_one_group_at_any_positive_length_and_singletons_at_zero():
    n = 2049
    a = gr.coincident(n, 700)
    for members in gr.MASKS:
        lo, hi = gr.span(members, n, 700)
        for length in (1e-45, 1e-20, 1.0):          # the smallest denormal included: q = +0 lies below every positive square
            (lab, k), p, m = host(a, members, length, count=True)
            assert k == 1 and np.all(lab[lo:hi] == lo) and gr.checker(lab, p, m, members, length), (members, length)
        (lab, k), p, m = host(a, members, 0.0, count=True)
        assert k == hi - lo and np.array_equal(lab[lo:hi], np.arange(lo, hi)) and gr.checker(lab, p, m, members, 0.0)


def test_a_nan_and_an_inf_particle_are_singletons_and_change_no_other_label():
    n, m = 300, 120
    a = world(n, m, seed=31, spread=3.0)
    length = gr.length_for(n)
    bad = [7, 130, 200, 201]
    clean_keep = np.setdiff1d(np.arange(n), bad)
    dirty = a.copy()
    dirty[7, 0], dirty[130, 1], dirty[200, 0], dirty[201, 0] = np.nan, np.inf, -np.inf, -np.inf          # two at -inf: their q is NaN
    for members in gr.MASKS:
        lab, p, m_ = host(dirty, members, length)
        assert m_ == m and gr.checker(lab, p, m, members, length)
        lo, hi = gr.span(members, n, m)
        for i in bad:
            assert lab[i] == (i if lo <= i < hi else gr.NONE)
            assert np.count_nonzero(lab == i) == (1 if lo <= i < hi else 0)          # nobody else is of its group
        # the world without those particles answers the same, index for index
        small, _, m_small = host(a[clean_keep], members, length)
        back = np.where(small == gr.NONE, np.uint32(gr.NONE), clean_keep[np.minimum(small, len(clean_keep) - 1)].astype(np.uint32))
        assert gr.same(lab[clean_keep], back), members


def test_a_poisoned_class_outside_the_mask_changes_no_bit_and_bridges_nothing():
    n, m = 300, 120
    a = world(n, m, seed=9, spread=3.0)
    length = gr.length_for(n)
    for members, lo, hi in ((gr.MASSIVE, m, n), (gr.MASSLESS, 0, m)):
        poisoned = a.copy()
        poisoned[lo:hi, 0:6] = np.nan
        if members == gr.MASSLESS:
            poisoned[lo:hi, 6] = 3.0e38          # huge masses
        clean, dirty = host(a, members, length)[0], host(poisoned, members, length)[0]
        assert gr.same(clean, dirty), members
        assert not gr.same(host(poisoned, gr.ALL, length)[0], host(a, gr.ALL, length)[0])          # ... and asked for, it is read
    bridge = gr.blank(3, 2)
    bridge[:, 0] = [0.0, 2.0, 1.0]          # massive at 0 and 2, a massless particle between them
    assert list(host(bridge, gr.MASSIVE, 1.5)[0]) == [0, 1, gr.NONE]
    assert list(host(bridge, gr.ALL, 1.5)[0]) == [0, 0, 0]
    assert list(host(bridge, gr.MASSLESS, 1.5)[0]) == [gr.NONE, gr.NONE, 2]


# ---- the helpers, on a case written out by hand --------------------------------------------------------------------------------

def test_n_groups_and_the_numpy_helpers_on_a_case_written_out_by_hand():
    a = gr.blank(8, 6)
    a[:, 0] = [0.0, 10.0, 1.0, 11.0, 2.0, 30.0, 10.5, 3.0]          # {0, 2, 4, 7} along x = 0 .. 3, {1, 3, 6} about x = 10, {5} alone
    a[:, 6] = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 0.0, 0.0]
    (lab, k), p, m = host(a, linking_length=1.25, count=True)
    assert m == 6 and np.array_equal(p[:, 0], a[:, 0])
    assert list(lab) == [0, 1, 0, 1, 0, 5, 1, 0] and k == 3 and isinstance(k, int)
    roots, sizes, sums = nb.group_table(lab, weights=p[:, 6])
    assert list(roots) == [0, 1, 5] and list(sizes) == [4, 3, 1] and list(sums) == [21.0, 10.0, 32.0]
    assert roots.dtype == np.uint32 and sizes.dtype == np.int64 and sums.dtype == np.float64
    assert [list(v) for v in nb.group_table(lab, min_members=2)] == [[0, 1], [4, 3]]
    assert list(nb.group_members(lab, 1)) == [1, 3, 6] and list(nb.group_members(lab, 5)) == [5] and list(nb.group_members(lab, 2)) == []
    (lab, k), _, _ = host(a, gr.MASSIVE, 1.25, count=True)
    assert list(lab) == [0, 1, 0, 1, 0, 5, gr.NONE, gr.NONE] and k == 3 and nb.NB_GROUP_NONE == gr.NONE
    roots, sizes = nb.group_table(lab)
    assert list(roots) == [0, 1, 5] and list(sizes) == [3, 2, 1]          # NB_GROUP_NONE is in no group; ties by root ascending below
    assert [list(v) for v in nb.group_table(np.array([3, 1, 1, 3], dtype=np.uint32))] == [[1, 3], [2, 2]]
    assert nb.linking_length_for(100, 25.0) == pytest.approx(0.2 * 0.5) and nb.linking_length_for(4, 16.0, b=1.0) == 2.0
    for bad in (dict(n=0, area=1.0), dict(n=5, area=0.0), dict(n=5, area=1.0, b=-1.0)):
        with pytest.raises(ValueError):
            nb.linking_length_for(**bad)
    with pytest.raises(ValueError):
        nb.group_table(np.zeros((2, 2), dtype=np.uint32))
    with pytest.raises(ValueError):
        nb.group_table(lab, weights=np.ones(3))


# ---- return conventions and ensembles on the host ------------------------------------------------------------------------------

def test_return_conventions_for_a_world_a_uniform_ensemble_and_a_ragged_one():
    a = world(250, 100, seed=1, spread=3.0)
    length = gr.length_for(250)
    w = nb.World(a)
    lab = w.groups(length)
    both = w.groups(length, "all", True)
    w.close()
    assert isinstance(lab, np.ndarray) and lab.dtype == np.uint32 and lab.shape == (250,)
    assert isinstance(both, tuple) and gr.same(both[0], lab) and type(both[1]) is int and both[1] == gr.count(lab)
    states = np.stack([world(250, 100, seed=s, spread=3.0) for s in range(3)])
    uniform = nb.WorldBatch(states)
    lab, k = uniform.groups(length, return_count=True)
    assert gr.same(uniform.groups(length, members=nb.NB_NEIGH_ALL), lab)          # integers pass through
    uniform.close()
    assert lab.dtype == np.uint32 and lab.shape == (3, 250) and k.dtype == np.uint32 and k.shape == (3,)
    for b in range(3):
        assert gr.same(lab[b], gr.model(states[b], 100, gr.ALL, length)) and k[b] == gr.count(lab[b])
    members = [world(n, m, seed=40 + n, spread=3.0) for n, m in ((1, 1), (2, 0), (333, 0), (257, 257), (700, 350))]
    members[4][5, 0] = np.nan
    wb = nb.WorldBatch.ragged(members)
    for mask in gr.MASKS:
        lab, k = wb.groups(1.0, gr.NAMES[mask], return_count=True)
        assert isinstance(lab, list) and len(lab) == 5 and k.dtype == np.uint32 and k.shape == (5,)
        for b, part in enumerate(members):
            alone, p, m = host(part, mask, 1.0)
            assert lab[b].flags.owndata and lab[b].dtype == np.uint32 and lab[b].shape == (len(part),)
            assert gr.same(lab[b], alone) and gr.checker(alone, p, m, mask, 1.0) and k[b] == gr.count(alone), (mask, b)
    assert isinstance(wb.groups(1.0), list)
    wb.close()
    # neighbouring members on top of one another share no group
    twin = nb.WorldBatch(np.stack([gr.coincident(5), gr.coincident(5)]))
    lab, k = twin.groups(1.0, return_count=True)
    twin.close()
    assert not lab.any() and list(k) == [1, 1]


def test_cpu_only_worlds_and_batches_never_open_a_device():
    code = ("import os, numpy as np, nbody_amd as nb, group_ref as gr\n"
            "from paircount_ref import world\n"
            "a = world(600, 300, seed=1, spread=3.0)\n"
            "w = nb.World(a); w.update_cpu(0.01, 2); got = w.groups(0.3); p = w.particles(); w.close()\n"
            "ok = gr.same(got, gr.model(p, 300, gr.ALL, 0.3))\n"
            "wb = nb.WorldBatch(np.stack([a, a])); gb = wb.groups(0.3, 'massive', True); wb.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', ok, got.shape, len(gb), gb[0].shape, gb[1].shape)\n")
    r = child(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK True (600,) 2 (2, 600) (2,)"


# ---- argument checks -----------------------------------------------------------------------------------------------------------

SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); wb = nb.WorldBatch(np.stack([a, a, a])); L = nb.nbody_lib(); H = nb.hip_lib()\n"
         "g = np.zeros(64, dtype=np.uint32); k = np.zeros(8, dtype=np.uint32)\n"
         "G, K = g.ctypes.data, k.ctypes.data\n"
         "s = nb.SimPipeline(4, 4); sb = nb.SimBatch(4, [4, 4, 4])\n"
         "def spec(members=3, length=1.0):\n"
         "    return C.byref(nb.WorldGroupSpec(members, length))\n")
SHARDED = "fn = nb.ALLGATHER_FN(lambda *x: None); ws = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
MEMBERS = "members must be a non-empty set of NB_NEIGH_MASSIVE | NB_NEIGH_MASSLESS"
FINITE, NEGATIVE = "linking_length must be finite", "linking_length must not be negative"
ABORTS = [
    # the World layer
    ("world NULL world", "L.GetWorldGroups(None, spec(), G, K)", "NULL argument"),
    ("world NULL spec", "L.GetWorldGroups(w._h, None, G, K)", "NULL argument"),
    ("world NULL group", "L.GetWorldGroups(w._h, spec(), None, K)", "NULL argument"),
    ("world members 0", "w.groups(1.0, members=0)", MEMBERS),
    ("world members 4", "w.groups(1.0, members=4)", MEMBERS),
    ("world members 7", "w.groups(1.0, members=7)", MEMBERS),
    ("world length NaN", "w.groups(float('nan'))", FINITE),
    ("world length inf", "w.groups(float('inf'))", FINITE),
    ("world length negative", "w.groups(-0.5)", NEGATIVE),
    ("sharded world", SHARDED + "L.GetWorldGroups(ws, spec(), G, K)", "GetWorldGroups of a sharded pipeline needs a collective"),
    # the batch layer
    ("batch NULL batch", "L.GetWorldBatchGroups(None, spec(), G, K)", "GetWorldBatchGroups: NULL argument"),
    ("batch NULL spec", "L.GetWorldBatchGroups(wb._h, None, G, K)", "GetWorldBatchGroups: NULL argument"),
    ("batch NULL group", "L.GetWorldBatchGroups(wb._h, spec(), None, None)", "GetWorldBatchGroups: NULL argument"),
    ("batch members 8", "wb.groups(1.0, members=8)", MEMBERS),
    ("batch members 0", "wb.groups(1.0, members=0)", MEMBERS),
    ("batch length NaN", "wb.groups(float('nan'))", FINITE),
    ("batch length negative", "wb.groups(-1.0)", NEGATIVE),
    # the seam: every check comes before any device touch (no device is visible to these children)
    ("seam NULL pipeline", "H.nb_hip_groups(None, 3, 1.0, G, K)", "NULL pipeline"),
    ("seam NULL group", "H.nb_hip_groups(s._h, 3, 1.0, None, K)", "nb_hip_groups: NULL argument"),
    ("seam members 0", "s.groups(1.0, members=0)", MEMBERS),
    ("seam members 5", "s.groups(1.0, members=5)", MEMBERS),
    ("seam length NaN", "s.groups(float('nan'))", FINITE),
    ("seam length -inf", "s.groups(float('-inf'))", FINITE),
    ("seam length negative", "s.groups(-1e-30)", NEGATIVE),
    ("seam before set_data", "s.groups(1.0)", "nb_hip_groups before SetSimulationData"),
    ("ensemble NULL ensemble", "H.nb_hip_ensemble_groups(None, 3, 1.0, G, K)", "NULL ensemble"),
    ("ensemble NULL group", "H.nb_hip_ensemble_groups(sb._h, 3, 1.0, None, K)", "nb_hip_ensemble_groups: NULL argument"),
    ("ensemble members 0", "sb.groups(1.0, members=0)", MEMBERS),
    ("ensemble members 16", "sb.groups(1.0, members=16)", MEMBERS),
    ("ensemble length inf", "sb.groups(float('inf'))", FINITE),
    ("ensemble length negative", "sb.groups(-2.0)", NEGATIVE),
    ("ensemble before set_data", "sb.groups(1.0)", "nb_hip_ensemble_groups before nb_hip_batch_set_data"),
    ("ragged ensemble before set_data", "nb.SimBatch.ragged([4, 9], [1, 2]).groups(1.0)", "nb_hip_ensemble_groups before nb_hip_batch_set_data"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_a_null_count_is_allowed_and_a_negative_zero_length_is_zero():
    r = child(SETUP + "L.GetWorldGroups(w._h, spec(length=1.5), G, None); a1 = [int(v) for v in g[:4]]\n"
              "L.GetWorldBatchGroups(wb._h, spec(length=-0.0), G, K)\nprint('SURVIVED', a1, [int(v) for v in g[:12]], [int(v) for v in k[:3]])")
    assert r.returncode == 0 and r.stdout.strip() == "SURVIVED [0, 0, 0, 0] [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3] [4, 4, 4]", (r.stdout, r.stderr)


def test_python_arguments_raise_before_the_library_is_called():
    w = nb.World(world(8, 8))
    for bad in ("mm", "heavy", None, ("massive",), 1.5, True):
        with pytest.raises(ValueError, match='members must be "massive", "massless" or "all"'):
            w.groups(1.0, members=bad)
    w.close()


# ---- sources, headers, exports -------------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_group.h") == ["GetWorldGroups"]
    assert declared_functions("nbody_batch_group.h") == ["GetWorldBatchGroups"]
    funcs, seam = {"GetWorldGroups", "GetWorldBatchGroups"}, {"nb_hip_groups", "nb_hip_ensemble_groups"}
    assert funcs <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert funcs <= have and "nb_cpu_groups" not in have, so          # the host path is internal
    assert seam <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and seam <= exported(nb.HIP_SO) and not seam & set(nb.TUNE_API)
    assert "nb_hip_group_span" in nb.TUNE_API and "nb_hip_group_span" in exported(nb.HIP_SO)
    assert "nb_hip_group_span" not in declared_functions("nbody_hip.h") and "nb_hip_group_span" not in nb.HIP_API
    assert nb.hip_lib().nb_hip_group_span(0) == 0          # auto unless a test says otherwise; host code only
    assert nb.hip_lib().nb_hip_version() == 400          # no version bump: the new surface is detected by its symbols
    text = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert 'dlsym "nb_hip_groups"' in text and 'dlsym "nb_hip_ensemble_groups"' in text
    header = open(os.path.join(ROOT, "include", "nbody_group.h")).read()
    assert "#define NB_GROUP_NONE 0xFFFFFFFFu" in header and '#include "nbody_neighbour.h"' in header and nb.NB_GROUP_NONE == 0xFFFFFFFF
    for word in ("periodic boundaries", "linking length per member", "velocity-space (6-D) linking", "unbinding of group",
                 "traced update", "sharded pipelines and Worlds"):
        assert word in " ".join(header.split()).replace(" * ", " "), word          # what is not built is said
    assert "linking length per member is not built" in " ".join(open(os.path.join(ROOT, "include", "nbody_batch_group.h")).read().split())
    # written once: one function object on the four classes, in no class's own namespace
    from nbody_amd.reads import ENTRY_POINTS, Reads
    for cls in (nb.SimPipeline, nb.World, nb.SimBatch, nb.WorldBatch):
        assert cls.groups is Reads.groups and "groups" not in vars(cls), cls
    assert ENTRY_POINTS["groups"] == ("nb_hip_groups", "nb_hip_ensemble_groups", "GetWorldGroups", "GetWorldBatchGroups")
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\bgroup\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\bgroup_cpu\.c", make, re.M)
    assert re.search(r"^\$\(OUT\)/%\.o:.*\$\(HERE\)group_common\.h", make, re.M) and "-ffp-contract=off" in make
    # the statement is written once: neither path restates q, the range of the mask or the union-find
    for source in ("group.hip", "group_cpu.c"):
        body = open(os.path.join(csrc, source)).read()
        assert '#include "group_common.h"' in body and "nb_pair_q(" in body and "nb_group_find(" in body and "nb_group_unite(" in body, source
        assert "dx * dx" not in body and "atomicCAS" not in body and "__atomic_" not in body, source
    assert "nb_neigh_range(" in open(os.path.join(csrc, "group.hip")).read()
    common = open(os.path.join(csrc, "group_common.h")).read()
    assert '#include "paircount_common.h"' in common and '#include "neighbour_common.h"' in common and "dx * dx" not in common
    for op in ("NB_GROUP_LOAD", "NB_GROUP_CAS", "NB_GROUP_MIN"):
        assert common.count("#define " + op) == 2, op          # one statement over three operations, device and host
    assert "__HIP_MEMORY_SCOPE_AGENT" in common and "__ATOMIC_RELAXED" in common


# ---- static ISA of group.hip ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def group_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("group_isa"), "group.hip")


def test_group_hip_holds_its_three_kernels_without_scratch_or_lds_within_the_registers_its_header_states(group_isa):
    source = open(os.path.join(ROOT, "nbody_amd", "csrc", "group.hip")).read()
    stated = {"group_pairs_kernel": int(re.search(r"group_pairs_kernel at most (\d+) VGPRs \((\d+) as built\)", source).group(1)),
              "group_init_kernel": int(re.search(r"group_init_kernel and group_flatten_kernel at most (\d+)", source).group(1))}
    stated["group_flatten_kernel"] = stated["group_init_kernel"]
    built = int(re.search(r"group_pairs_kernel at most (\d+) VGPRs \((\d+) as built\)", source).group(2))
    meta = kernel_meta(group_isa)
    assert sorted(next(k for k in stated if k in m[0]) for m in meta) == sorted(stated), [m[0] for m in meta]          # these and no others
    for name, scratch, sgpr, vgpr in meta:
        kernel = next(k for k in stated if k in name)
        print(f"[group isa] {kernel}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs (stated: at most {stated[kernel]})")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgpr <= stated[kernel] <= 64, (name, vgpr)          # 64: eight waves per SIMD, four workgroups of eight waves per CU
        if kernel == "group_pairs_kernel":
            assert vgpr <= built, (vgpr, built)          # the as-built number of the header is no flattery
    assert sorted(re.findall(r"\.max_flat_workgroup_size:\s+(\d+)", group_isa)) == ["256", "256", "512"]
    assert set(re.findall(r"\.group_segment_fixed_size:\s+(\d+)", group_isa)) == {"0"}          # no LDS, as the header says


def test_q_is_formed_by_multiplies_and_an_add_never_by_an_fma(group_isa):
    bodies = {name: body for name, body in functions(group_isa).items() if "group_pairs_kernel" in name}
    assert len(bodies) == 1
    for name, body in bodies.items():
        ops = [ins.split()[0] for ins in body]
        muls = sum(op.startswith(("v_mul_f32", "v_pk_mul_f32")) for op in ops)
        adds = sum(op.startswith(("v_add_f32", "v_pk_add_f32")) for op in ops)
        subs = sum(op.startswith(("v_sub_f32", "v_subrev_f32", "v_pk_add_f32")) for op in ops)
        print(f"[group isa] {name}: {muls} multiplies, {adds} adds, {subs} subtractions")
        assert muls > 0 and adds > 0 and subs > 0, name
        fused = [ins for ins in body if re.match(r"v_(pk_)?(fma|fmac|mad|mac)\w*_f(16|32|64)", ins)]
        assert not fused, (name, fused)          # q is the kernel's only float arithmetic: any fma would be feeding it
