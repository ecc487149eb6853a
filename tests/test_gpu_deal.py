"""Dealt launches ("deal" hook; nbody_amd/csrc/kernels.hip dealt_kernel) against classic launches of the same shape: a dealt
launch computes the same (receiver tile, source part) items with the same code, the finish kernel adds the same parts in
the same order, so the full state (pos, vel, acc, statics) after any sequence of calls is bit-identical with deal = 0.
The shapes are the smallest at which a dealt launch can go wrong: fewer items than resident slots, tail lanes and a tile
count that is no multiple of eight, the acc[] chain of source passes, cached graphs and their replays, an upload in
mid-sequence, the knob flipped on a live pipeline -- and one row where auto itself deals.  Nothing is timed."""
import numpy as np  # noqa: F401
import pytest

import nbody_amd as nb
from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

DT = 0.01


def pipeline(part, m, **knobs):
    sim = nb.SimPipeline(part.shape[0], m)
    sim.configure(**knobs)
    sim.set_data(part)
    return sim


def same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n,knobs,items", [
    (1000, dict(k=1, w=16, split=1), 16),                          # every workgroup resident at once; the kernel integrates itself
    (1001, dict(k=2, w=16, split=2, unit=8, passes=2), 16),        # tail lanes, 8 tiles + 1 receiver, acc[] chain, finish kernel
    (1001, dict(k=2, w=16, split=16, unit=8, passes=2), 128),
])
def test_forced_dealt_launches_equal_classic_ones(n, knobs, items):
    part, m = synth(n, 0.5, seed=n)
    for graph in (0, 1):
        classic = pipeline(part, m, deal=0, lanes=1, fused_finish=0, fused_chain=0, graph=graph, **knobs)
        dealt = pipeline(part, m, deal=1, lanes=1, fused_finish=0, fused_chain=0, graph=graph, **knobs)
        for steps in (1, 3, 4):
            classic.update(steps, DT)
            dealt.update(steps, DT)
            assert dealt.last_deal() == (True, items, max(8, items // 32)) and classic.last_deal()[0] is False
            assert dealt.deal_counter() == 0
            assert same(dealt.get_data(), classic.get_data()), (n, knobs, graph, steps)
        assert dealt.launch_shape() == classic.launch_shape()      # workgroups stays the item count
        classic.close()
        dealt.close()


def test_plain_steps_cached_chains_replays_and_an_upload_in_mid_sequence():
    """N = 20 000 with the fused finish off: 5 plain steps, a 32-step chain three times (built, replayed, replayed), a second
    state uploaded in mid-sequence, more steps; the counter reads zero after every call.  k, split and unit are left on auto;
    w is pinned to 16, because auto picks eight waves per workgroup at this size (k = 2, w = 8, split = 8) and only the
    sixteen-wave kernels have a dealt instantiation."""
    part, m = synth(20000, 0.5, seed=5)
    other = part.copy()
    other[:, 0:4] *= np.float32(1.25)             # a second state of the same world (same masses, same partition)
    classic = pipeline(part, m, deal=0, fused_finish=0, w=16)
    dealt = pipeline(part, m, deal=1, fused_finish=0, w=16)
    for sim in (classic, dealt):
        sim.update(1, DT)
    assert dealt.deal_counter() == 0              # between two plain launches
    for sim in (classic, dealt):
        sim.update(4, DT)
    assert dealt.last_deal()[0] and not classic.last_deal()[0] and dealt.deal_counter() == 0
    assert dealt.launch_shape() == classic.launch_shape()
    assert same(dealt.get_data(), classic.get_data())
    for sim in (classic, dealt):
        sim.configure(graph=1)
    for call in range(3):                         # the third call replays the cached graph
        classic.update(32, DT)
        dealt.update(32, DT)
        assert dealt.deal_counter() == 0 and dealt.last_deal()[0], call
        assert same(dealt.get_data(), classic.get_data()), call
    assert dealt.graph_stats()["cached"] == classic.graph_stats()["cached"] == 1
    for sim in (classic, dealt):
        sim.set_data(other)
        sim.update(3, DT)
        sim.update(32, DT)
    assert dealt.deal_counter() == 0
    assert same(dealt.get_data(), classic.get_data())
    classic.close()
    dealt.close()


def test_flipping_the_knob_on_a_live_pipeline_equals_fresh_pipelines():
    part, m = synth(5000, 0.5, seed=9)
    knobs = dict(k=2, w=16, split=4, lanes=1, fused_finish=0, graph=1)
    live = pipeline(part, m, deal=1, **knobs)
    state = part
    for call, (deal, steps) in enumerate(((1, 20), (0, 20), (1, 20), (1, 3), (0, 1))):
        live.configure(deal=deal)
        live.update(steps, DT)
        assert live.last_deal()[0] == bool(deal) and live.deal_counter() == 0
        fresh = pipeline(state, m, deal=0, **knobs)
        fresh.update(steps, DT)
        state = fresh.get_data()
        fresh.close()
        assert same(live.get_data(), state), (deal, steps)
        if call == 2:   # a dealt and a classic 20-step chain are two cached graphs, neither re-patched nor rebuilt
            assert live.graph_stats()["cached"] == 2
    live.close()


def test_auto_deals_the_headline_size_and_the_bits_stay():
    """deal = 2 deals from 32 resident rounds on: N = 2^20 is the smallest BASELINE size it takes (262 144 is 8 rounds and
    stays classic), so the row where auto itself deals is two steps there."""
    n = 1 << 20
    part, m = synth(n, 0.5, seed=20)
    assert nb.plan_deal(n, m) and not nb.plan_deal(262144, 131072)
    classic = pipeline(part, m, deal=0)
    classic.update(2, DT)
    want = classic.get_data()
    assert classic.last_deal()[0] is False
    classic.close()
    auto = pipeline(part, m, deal=2)
    auto.update(2, DT)
    dealt, items, extra = auto.last_deal()
    assert dealt and items == auto.launch_shape()["workgroups"] and extra == items // 32
    assert auto.deal_counter() == 0
    assert same(auto.get_data(), want)
    auto.close()
    small, ms = synth(30000, 0.5, seed=21)
    sim = pipeline(small, ms, deal=2)
    sim.update(2, DT)
    assert sim.last_deal()[0] is False            # far below 32 rounds: auto leaves it alone
    sim.close()
