"""group_pairs_kernel (group.hip) where its own index arithmetic and its kept roots can go wrong, on the GPU: the mask range
[lo, hi) on, before and behind every tile (128), block (256), slice (32) and fetch (8) edge of the walk with a planted link across
each (tests/group_edge_cases.py; the premise is held on the CPU by tests/test_group_cpu_edges.py), for a pipeline and for ragged
and uniform ensembles, at the automatic span and at forced ones; the worlds in which every hook of a launch meets in one tree at
every forced span length; and hand-placed worlds for the two receivers a lane holds.  Every comparison is of raw bits."""
import numpy as np
import pytest

import group_edge_cases as ge
import group_ref as gr
import nbody_amd as nb

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


class forced_span:
    """nb_hip_group_span(blocks) for the block, auto (0) behind it whatever happens inside."""

    def __init__(self, blocks):
        self.blocks = blocks

    def __enter__(self):
        nb.hip_lib().nb_hip_group_span(self.blocks)

    def __exit__(self, *exc):
        assert nb.hip_lib().nb_hip_group_span(0) == self.blocks


def pipeline(a, m):
    sim = nb.SimPipeline(a.shape[0], m)
    sim.set_data(a)
    return sim


# ---- the mask range at every edge of the walk -----------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ge.MASS_LENS)
def test_the_mask_range_on_before_and_behind_every_edge_of_the_walk(m):
    n = ge.N
    sim = nb.SimPipeline(n, m)
    for members in gr.MASKS:
        lo, hi = gr.span(members, n, m)
        outside = np.ones(n, dtype=bool)
        outside[lo:hi] = False
        for length in ge.LENGTHS:
            a, _ = ge.edge_world(n, m, members, length)
            want = gr.model(a, m, members, length)
            host = nb.World(a)          # never stepped: the host path
            assert host.particles().tobytes() == a.tobytes()
            on_host, k_host = host.groups(length, gr.NAMES[members], return_count=True)
            host.close()
            assert gr.same(on_host, want) and k_host == gr.count(want), (m, members, length, "host path against the model")
            sim.set_data(a)
            for blocks in ge.SPANS:          # the span offsets start from r0 / 256
                with forced_span(blocks):
                    got, k = sim.groups(length, gr.NAMES[members], return_count=True)
                assert gr.same(got, want), (m, members, length, blocks, "device against the model")
                assert type(k) is int and k == k_host, (m, members, length, blocks, "n_groups")
                assert np.all(got[outside] == gr.NONE) and np.all(got[lo:hi] <= np.arange(lo, hi)), (m, members, length, blocks)
    sim.close()


def check_ensemble(batch, states, mass_lens, members, length, label):
    name = gr.NAMES[members]
    want = [gr.model(a, m, members, length) for a, m in zip(states, mass_lens)]
    alone = []
    for a, m in zip(states, mass_lens):
        sim = pipeline(a, m)
        alone.append(sim.groups(length, name, return_count=True))
        sim.close()
    for blocks in (0, 1):
        with forced_span(blocks):
            got, k = batch.groups(length, name, return_count=True)
        for b in range(len(states)):
            assert gr.same(got[b], want[b]), (label, name, length, blocks, b, "ensemble against the model")
            assert gr.same(got[b], alone[b][0]) and k[b] == alone[b][1] == gr.count(want[b]), (label, name, length, blocks, b, "its own pipeline")


def test_a_ragged_ensemble_whose_members_stand_on_the_edges():
    sizes, mass_lens = ge.RAGGED
    batch = nb.SimBatch.ragged(sizes, mass_lens)
    for members in gr.MASKS:
        for length in ge.LENGTHS:
            states = ge.ensemble_states(sizes, mass_lens, members, length)
            batch.set_data(states)
            check_ensemble(batch, states, mass_lens, members, length, "ragged")
    batch.close()


def test_a_uniform_ensemble_whose_members_stand_on_the_edges():
    n, mass_lens = ge.UNIFORM
    batch = nb.SimBatch(n, list(mass_lens))
    for members in gr.MASKS:
        for length in ge.LENGTHS:
            states = ge.ensemble_states([n] * len(mass_lens), mass_lens, members, length)
            batch.set_data(np.stack(states))
            check_ensemble(batch, states, mass_lens, members, length, "uniform")
    batch.close()


# ---- every hook in one tree, at every span --------------------------------------------------------------------------------------

ONE_TREE = {
    "coincident, the smallest denormal": (lambda: gr.coincident(2049, 700), 700, 1e-45),
    "coincident, 1": (lambda: gr.coincident(2049, 700), 700, 1.0),
    "chain, above the spacing": (lambda: gr.chain(2049, seed=2050, m=1024)[0], 1024, gr.above(1.0)),
    "chain, on the spacing": (lambda: gr.chain(2049, seed=2050, m=1024)[0], 1024, 1.0),
    "lattice, above the spacing": (lambda: gr.lattice(45, m=1000), 1000, gr.above(1.0)),
}


@pytest.mark.parametrize("name", sorted(ONE_TREE))
def test_worlds_that_percolate_give_the_model_at_every_forced_span_length(name):
    """Blocks of 256 sources: N = 2 049 has 9.  A span of 1 is one workgroup per (tile, block), 2, 3 and 5 leave ragged last spans,
    1000 is one workgroup per tile.  Where everything links every hook of the launch meets in one tree; three calls each."""
    make, m, length = ONE_TREE[name]
    a = make()
    sim = pipeline(a, m)
    want = {members: gr.model(a, m, members, length) for members in gr.MASKS}
    if "on the spacing" in name:
        assert gr.count(want[gr.ALL]) == len(a)          # q = 1 is not < 1: nothing links
    else:
        assert gr.count(want[gr.ALL]) == 1 and not want[gr.ALL].any()
    for blocks in (0, 1, 2, 3, 5, 1000):
        with forced_span(blocks):
            for members in gr.MASKS:
                for call in range(3):
                    got, k = sim.groups(length, gr.NAMES[members], return_count=True)
                    assert gr.same(got, want[members]) and k == gr.count(want[members]), (name, blocks, members, call)
    sim.close()


def test_six_thousand_coincident_particles_against_the_host_path():
    n, m = 6000, 2000
    a = gr.coincident(n, m)
    sim, host = pipeline(a, m), nb.World(a)
    for members in gr.MASKS:
        lo, hi = gr.span(members, n, m)
        expected = np.full(n, gr.NONE, dtype=np.uint32)
        expected[lo:hi] = lo
        got, k = sim.groups(1.0, gr.NAMES[members], return_count=True)
        assert gr.same(got, expected) and k == 1, members
        assert gr.same(host.groups(1.0, gr.NAMES[members]), expected), members
    sim.close()
    host.close()


# ---- the two receivers of a lane ------------------------------------------------------------------------------------------------
# A lane of tile t holds receivers 128 t + l and 128 t + 64 + l, shares one find per source between them and keeps a root for each.
# Worlds placed by hand at a linking length of 1: particles of a structure stand in a row 0.75 apart (neighbours link, any others are
# 1.5 apart or more), lane l's structure at x = 20 l, every particle that is in no structure alone on a far row.

STEP, LENGTH = 0.75, 1.0


def hand_world(n, rows):
    """rows: lists of indices standing in a row 0.75 apart, row r about x = 20 r; everyone else alone at (5 i, 500)."""
    a = gr.blank(n)
    a[:, 0], a[:, 1] = 5.0 * np.arange(n), 500.0
    for r, row in enumerate(rows):
        for k, i in enumerate(row):
            a[i, 0], a[i, 1] = 20.0 * r + STEP * k, 0.0
    assert len({i for row in rows for i in row}) == sum(len(row) for row in rows)
    return a


def same_source_from_different_trees():
    """N = 256, tile 1: receivers 128 + l and 192 + l both link to source l of block 0 and not to one another: the one find of
    the source serves two receivers that are still their own trees."""
    rows = [[128 + l, l, 192 + l] for l in range(64)]
    want = np.arange(256, dtype=np.uint32)
    want[128:192] = np.arange(64)
    want[192:256] = np.arange(64)
    return hand_world(256, rows), want


def two_sources_of_one_fetch_behind_a_joining_fetch():
    """N = 384, tile 2 (receivers 256 + l and 320 + l), sources of block 0.  Wave w walks sources 32 w .. 32 w + 31 and lanes
    8 w .. 8 w + 7 have theirs there: fetch 0 of the slice holds c, to which both receivers link (their trees join); a later fetch
    of the same wave holds a and b side by side, a linked to the first receiver only and b to the second."""
    rows, want = [], np.arange(384, dtype=np.uint32)
    for l in range(64):
        w, u = divmod(l, 8)
        base = 32 * w
        c = base + u
        a = base + 8 + 2 * u if u < 4 else base + 16 + 2 * (u - 4)
        rows.append([a, 256 + l, c, 320 + l, a + 1])
        want[[a, a + 1, 256 + l, 320 + l]] = c
    return hand_world(384, rows), want


def two_sources_joined_only_by_a_later_block():
    """N = 384, tile 2, lanes 32 .. 63 (u = l - 32): in block 0 the first receiver links to a = 2 u and the second to b = 2 u + 1,
    side by side in one fetch and in different trees; only the diagonal block holds d = 256 + u, below both receivers, to which
    both link."""
    rows, want = [], np.arange(384, dtype=np.uint32)
    for u in range(32):
        l = 32 + u
        rows.append([2 * u, 256 + l, 256 + u, 320 + l, 2 * u + 1])
        want[[2 * u + 1, 256 + l, 256 + u, 320 + l]] = 2 * u
    return hand_world(384, rows), want


def a_source_of_the_lanes_own_tile():
    """N = 256: receiver 64 + l links to source l and receiver 192 + l to source 128 + l -- the other receiver of the same lane,
    in the masked diagonal block (j < i)."""
    rows = [[l, 64 + l] for l in range(64)] + [[128 + l, 192 + l] for l in range(64)]
    want = np.arange(256, dtype=np.uint32)
    want[64:128] = np.arange(64)
    want[192:256] = np.arange(128, 192)
    return hand_world(256, rows), want


@pytest.mark.parametrize("make", [same_source_from_different_trees, two_sources_of_one_fetch_behind_a_joining_fetch,
                                  two_sources_joined_only_by_a_later_block, a_source_of_the_lanes_own_tile])
def test_the_two_receivers_of_a_lane(make):
    a, by_hand = make()
    n = len(a)
    assert gr.same(gr.model(a, n, gr.ALL, LENGTH), by_hand), "the labels written out by hand against the model"
    host = nb.World(a)
    assert host.particles().tobytes() == a.tobytes() and gr.same(host.groups(LENGTH), by_hand), "host path"
    host.close()
    sim = pipeline(a, n)
    for blocks in (0, 1, 2, 1000):          # auto is one block a workgroup here; 2 and 1000 walk both blocks in one workgroup
        with forced_span(blocks):
            for call in range(3):
                got, k = sim.groups(LENGTH, return_count=True)
                assert gr.same(got, by_hand) and k == gr.count(by_hand), (make.__name__, blocks, call)
    sim.close()
