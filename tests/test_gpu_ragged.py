"""Ragged world ensembles on the GPU (nb.SimBatch.ragged / nb.WorldBatch.ragged): member b of an ensemble whose members
differ in size is BIT-IDENTICAL -- particles, energy, potential, every row of a traced call -- to the same particles as the
single member of a uniform SimBatch(N_b, [M_b]), whatever its index, its neighbours, their sizes, their step sizes or the
launch groups present are.  (tests/test_gpu_batch.py holds that uniform member to a pinned SimPipeline.)

One ensemble covers every path: the three launch groups interleaved, each group's largest member not first (so workgroups
that leave early occur), sizes on both sides of every threshold (128 | 129, 256 | 257, 512 | 513, 1581 | 1582), M_b = 0, 1,
N_b and values that are no multiple of 8 or 256, and a step size per member.  Odd step counts (3, 5, 17) make the
lane-split groups end in the other position buffer than the chain group started in.  No tolerance anywhere."""
import struct

import numpy as np
import pytest

import nbody_amd as nb
from gpu_common import synth

pytestmark = pytest.mark.gpu

SIZES = [250, 1, 700, 129, 1582, 128, 513, 512, 2000, 257, 1581, 64]
MASS = [119, 1, 0, 129, 777, 1, 257, 300, 967, 100, 1581, 37]
CHAIN = [b for b, n in enumerate(SIZES) if n <= 512]          # the members of an all-chain ensemble
DTS = [0.01 * (1.0 + 0.1 * b) for b in range(len(SIZES))]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


_worlds = {}


def world(b, seed=0):
    """member b: SIZES[b] partitioned particles of which exactly MASS[b] are massive"""
    if (b, seed) not in _worlds:
        part, m = synth(SIZES[b], frac_massive=1.1, seed=7000 + 100 * seed + b)
        assert m == SIZES[b]
        part = part.copy()
        part[MASS[b]:, 6] = 0.0
        part[MASS[b]:, 7] = 0.5
        _worlds[(b, seed)] = part
    return _worlds[(b, seed)]


def ragged(members=None, seed=0, others_seed=None, keep=None):
    members = list(range(len(SIZES))) if members is None else members
    r = nb.SimBatch.ragged([SIZES[b] for b in members], [MASS[b] for b in members])
    r.set_data([world(b, seed if others_seed is None or b == keep else others_seed) for b in members])
    return r


def dts(members=None):
    return [DTS[b] for b in (range(len(SIZES)) if members is None else members)]


def ebits(e):
    flat = []
    for k in ("kinetic", "potential", "mass", "momentum", "angular_momentum", "center_of_mass"):
        v = e[k]
        flat += list(v) if isinstance(v, tuple) else [v]
    return struct.pack("<8d", *flat)


_alone = {}


def alone(b, calls):
    """member b as the single member of a uniform SimBatch through `calls` = (steps, ...):
    (particles, energy bits, potential) after them -- computed once, shared, never changed"""
    key = (b, tuple(calls))
    if key not in _alone:
        u = nb.SimBatch(SIZES[b], [MASS[b]])
        u.set_data(world(b)[None])
        for steps in calls:
            u.update(steps, DTS[b])
        _alone[key] = (u.get_data()[0], ebits(u.energy()[0]), u.potential()[0])
        u.close()
    return _alone[key]


def test_the_groups_are_what_the_sizes_say():
    r = ragged()
    shape = r.launch_shape()
    assert [(g["path"], g["w"], g["lanes"], g["members"]) for g in shape["groups"]] == \
        [("chain", 4, 1, 7), ("lanes", 8, 8, 3), ("lanes", 16, 4, 2)]
    # lane-split grids cover the group's largest member: 1581 -> 198 tiles of 8 receivers, 2000 -> 125 tiles of 16
    assert [g["workgroups"] for g in shape["groups"]] == [7, 3 * 198, 2 * 125]
    assert r.sizes() == SIZES
    r.close()


@pytest.mark.parametrize("calls", [(3,), (5, 12)], ids=["3", "5+12"])
def test_every_member_equals_its_own_uniform_ensemble(calls):
    r = ragged()
    for steps in calls:
        r.update(steps, dts())
    assert r.dt_uploads() == 1                    # the same step sizes again: no second upload, as update does
    got = r.get_data()
    one = [r.get_member(b) for b in range(len(SIZES))]
    r.close()
    for b in range(len(SIZES)):
        want = alone(b, (sum(calls),))[0]          # any cutting of the calls
        assert got[b].shape == (SIZES[b], 8)
        assert np.array_equal(got[b].view(np.uint8), want.view(np.uint8)), (b, SIZES[b], MASS[b], int((got[b] != want).sum()))
        assert one[b].tobytes() == want.tobytes(), b
    assert not np.array_equal(got[0][:, 0:2], world(0)[:, 0:2])       # it did move


def test_one_step_size_for_all_and_a_second_upload():
    members = [0, 2, 4, 3]
    r = ragged(members)
    r.update(2, DTS[0])
    r.update(1, DTS[0])
    assert r.dt_uploads() == 1
    r.update(2, [DTS[0]] * 3 + [DTS[3]])
    assert r.dt_uploads() == 2
    got = r.get_data()
    r.close()
    u = nb.SimBatch(SIZES[0], [MASS[0]])
    u.set_data(world(0)[None])
    u.update(5, DTS[0])
    assert got[0].tobytes() == u.get_data()[0].tobytes()
    u.close()


def test_energy_and_potential_are_bitwise_per_member_before_and_after_steps():
    r = ragged()
    for calls in ((), (3,)):
        if calls:
            r.step_async(3, dts())                # queued, not waited for: the diagnostics run behind it
        e, phi = r.energy(), r.potential()
        assert len(e) == len(phi) == len(SIZES)
        for b in range(len(SIZES)):
            _, want_e, want_phi = alone(b, calls)
            assert ebits(e[b]) == want_e, (b, calls, e[b])
            assert phi[b].shape == (SIZES[b],) and phi[b].tobytes() == want_phi.tobytes(), (b, calls)
    assert r.dt_uploads() == 1
    r.close()


@pytest.mark.parametrize("every", [5, 1])
@pytest.mark.parametrize("mixed", [False, True], ids=["all-chain", "mixed"])
def test_traced_updates_record_the_energy_of_separately_stepped_states(mixed, every):
    members = list(range(len(SIZES))) if mixed else CHAIN
    n = 12
    r = ragged(members)
    rows = r.trace(n, dts(members), every)
    info = r.last_trace_info()
    got = r.get_data()
    r.close()
    assert rows.shape == (1 + n // every, len(members), 8)
    if mixed:
        assert info["fused"] == 0                 # a lane-split member: the diagnostics launches are interleaved
    else:
        assert info == {"fused": 1, "launches": 1}
    for i, b in enumerate(members):
        for rec in range(rows.shape[0]):
            calls = (rec * every,) if rec else ()
            assert rows[rec, i].tobytes() == alone(b, calls)[1], (b, rec)
        assert got[i].tobytes() == alone(b, (n,))[0].tobytes(), b     # the trajectory is update(12)'s
    if not mixed:
        t = ragged(members)
        t.trace_mode(1)
        again = t.trace(n, dts(members), every)
        assert t.last_trace_info()["fused"] == 0
        assert again.tobytes() == rows.tobytes()
        assert all(a.tobytes() == g.tobytes() for a, g in zip(t.get_data(), got))
        t.close()


@pytest.mark.parametrize("n", [129, 513, 1582], ids=["chain-2-tiles", "lanes-8x8", "lanes-16x4"])
def test_a_ragged_ensemble_of_equal_sizes_is_the_uniform_ensemble(n):
    """Both come out of one constructor and one launch walk: the same launches through the other kernel family.  B = 3 with
    M = (N, 0, 77) and a step size per member; update(3), update(2), trace(5, every=2): everything observable is bitwise equal."""
    mass, steps = [n, 0, 77], [0.01, 0.013, 0.007]
    members = []
    for b, m in enumerate(mass):
        part = synth(n, frac_massive=1.1, seed=9100 + n + b)[0].copy()
        part[m:, 6] = 0.0
        part[m:, 7] = 0.5
        members.append(part)
    u, r = nb.SimBatch(n, mass), nb.SimBatch.ragged([n] * 3, mass)
    u.set_data(np.stack(members))
    r.set_data(members)
    seen = []
    for batch in (u, r):
        batch.update(3, steps)
        batch.update(2, steps)
        rows = batch.trace(5, steps, 2)
        seen.append((b"".join(np.asarray(a).tobytes() for a in batch.get_data()), b"".join(ebits(e) for e in batch.energy()),
                     b"".join(np.asarray(p).tobytes() for p in batch.potential()), rows.shape, rows.tobytes(),
                     batch.last_trace_info(), batch.dt_uploads()))
        batch.close()
    for name, a, b in zip(("get_data", "energy", "potential", "trace shape", "trace rows", "last_trace_info", "dt_uploads"), *seen):
        assert a == b, name
    assert seen[0][3] == (3, 3, 8) and seen[0][6] == 1 and seen[0][5]["fused"] == (1 if n <= 512 else 0)
    assert seen[0][0] != np.stack(members).tobytes()          # it did move


@pytest.mark.parametrize("keep", [0, 2, 8, 11])
def test_a_member_does_not_see_its_neighbours(keep):
    r = ragged(seed=0, others_seed=1, keep=keep)   # every other member holds different particles
    r.update(3, dts())
    got, e, phi = r.get_member(keep), r.energy()[keep], r.potential()[keep]
    r.close()
    want, want_e, want_phi = alone(keep, (3,))
    assert got.tobytes() == want.tobytes() and ebits(e) == want_e and phi.tobytes() == want_phi.tobytes()


def test_set_data_then_get_data_returns_the_input():
    r = ragged()
    got = r.get_data()
    for b in range(len(SIZES)):
        assert got[b].tobytes() == world(b).tobytes(), b
        assert r.get_member(b).tobytes() == world(b).tobytes(), b
    r.close()


def test_world_batch_ragged_steps_like_the_sim_batch():
    wb = nb.WorldBatch.ragged([world(b) for b in range(len(SIZES))])
    assert wb.sizes() == SIZES
    wb.update_gpu(dts(), 3)
    e, phi = wb.energy(), wb.potential()          # the device holds the newest state: device path
    for b in range(len(SIZES)):
        want, want_e, want_phi = alone(b, (3,))
        assert wb.member(b).tobytes() == want.tobytes(), b
        assert ebits(e[b]) == want_e and phi[b].tobytes() == want_phi.tobytes(), b
    rows = wb.update_gpu_traced(dts(), 2, 1)
    assert rows.shape == (3, len(SIZES), 8) and rows[0, 4].tobytes() == alone(4, (3,))[1]
    wb.close()
