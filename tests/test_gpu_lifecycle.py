"""Who frees what, on the MI355X: every device array and event of a SimPipeline / SimBatch is a member of an owner type
(nbody_amd/csrc/pipeline_internal.h DevBuf, DevEvent, Interval) and goes with the object.  nb.live_resources() counts both
kinds at their one seam, so each case is the same three lines: take the counts, make the object and call everything that
allocates lazily (the counts must have risen: the hook has teeth), close it, and the counts are back.  Against the counts
on entry, not zero: other test modules keep cached objects alive.  Every case runs twice in a row."""
import numpy as np
import pytest

import nbody_amd as nb
from gpu_common import synth

pytestmark = pytest.mark.gpu

DT = 0.01
ETA, DT_MAX = 0.1, 1.0


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def view(width, height):
    return nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 0.01, width, height, 100.0)


def world(n, m, seed=0):
    """n particles in the World's order, exactly the first m of them massive"""
    part, _ = synth(n, frac_massive=1.1, seed=seed + n)
    part[m:, 6] = 0.0
    part[m:, 7] = 0.5
    return part


def returns_what_it_took(make_and_use):
    for _ in range(2):
        base = nb.live_resources()
        obj = make_and_use()
        live = nb.live_resources()
        assert live[0] > base[0] and live[1] > base[1], (base, live)
        obj.close()
        assert nb.live_resources() == base


def used_pipeline(n, m, want_split):
    part = world(n, m)
    s = nb.SimPipeline(n, m)
    s.set_data(part)
    s.update(3, DT)
    s.update(40, DT)
    s.update(40, DT)      # the second use of a chain length: a cached graph
    if want_split:
        assert s.launch_shape()["split"] > 1      # parts and tickets exist
    s.energy()
    s.potential()
    points = part[:5, 0:2].copy()
    s.potential_at(points, 1.0)
    s.potential_map(view(16, 8), 1.0)
    s.acceleration_map(view(16, 8), 1.0)
    s.acceleration_at(points, 1.0)
    s.bounds()
    s.render_counts(view(16, 8))
    s.render(view(16, 8))
    s.render(view(32, 16))      # the count image and the frame regrow
    s.update_adaptive(4, ETA, DT_MAX)
    s.update_adaptive(200, ETA, DT_MAX, resume=True)      # the log outgrows its buffer: the regrow that carries the head
    s.update_leapfrog(2, DT)
    assert s.last_step_ms()[0] > 0.0      # the constructor turned the timing knob on
    return s


def test_small_pipeline_returns_every_buffer_and_event():
    """N = 300, M = 120: the one-workgroup chain and the canonical graph."""
    returns_what_it_took(lambda: used_pipeline(300, 120, False))


def test_split_pipeline_returns_every_buffer_and_event():
    """N = 3 001, all massive: the smallest size at which the source split really runs."""
    returns_what_it_took(lambda: used_pipeline(3001, 3001, True))


def used_batch(n, mass_lens):
    count = len(mass_lens)
    members = np.stack([world(n, m, seed=b) for b, m in enumerate(mass_lens)])
    s = nb.SimBatch(n, mass_lens)
    s.set_data(members)
    s.update(3, DT)
    s.update(3, [DT * (b + 1) for b in range(count)])
    s.trace(4, DT, 2)
    s.energy()
    s.potential()
    s.bounds()
    s.render_counts(view(16, 16))
    s.render(view(16, 16))
    s.render_mode(1)
    s.render(view(16, 16))      # the global path and its disc list
    s.update_adaptive(4, ETA, DT_MAX)
    s.update_adaptive(64, ETA, DT_MAX, resume=True)
    s.update_leapfrog(2, DT)
    s.get_data()
    return s


@pytest.mark.parametrize("n,mass_lens", [(250, [120] * 3), (600, [300] * 2)], ids=["chain", "lane-split"])
def test_ensemble_returns_every_buffer_and_event(n, mass_lens):
    returns_what_it_took(lambda: used_batch(n, mass_lens))


def used_ragged():
    sizes, mass_lens = [100, 600, 2000], [50, 300, 1000]      # one member per launch group: three device lists
    members = [world(n, m) for n, m in zip(sizes, mass_lens)]
    s = nb.SimBatch.ragged(sizes, mass_lens)
    s.set_data(members)
    s.update(3, DT)
    s.trace(4, DT, 2)
    s.energy()
    s.potential()
    s.get_data()
    return s


def test_ragged_ensemble_returns_every_buffer_and_event():
    returns_what_it_took(used_ragged)


def used_group():
    part = world(300, 120)
    g = nb.LocalShardGroup(300, 120, 2)      # the owned gathered arrays behind src_pos, the shared stream
    g.set_data(part)
    g.step(2, DT)
    g.get_data()
    return g


def test_local_shard_group_returns_every_buffer_and_event():
    returns_what_it_took(used_group)
