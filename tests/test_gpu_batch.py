"""World ensembles on the GPU (nb.SimBatch / nb.WorldBatch): member b of an ensemble is BIT-IDENTICAL to the same particles
stepped alone in a SimPipeline pinned to the ensemble's launch shape -- whatever B, its index, its neighbours, the call
cutting or the other members' step sizes are.  No tolerance is involved except where the golden fixtures are checked with
gpu_common's existing checkers.  No wall-clock assertions here (tests/test_gpu_batch_perf.py holds the only one)."""
import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
from gpu_common import DISPLACEMENT_TOL, check_one_step, matched_shape, rel_displacement, synth

pytestmark = pytest.mark.gpu

DT = 0.01
CHAIN_N = [1, 7, 64, 128, 129, 250, 256, 257, 512]
LANES_N = [513, 800, 1000, 2000, 3000]
CHECKED_OF_300 = 16        # besides the first and the last member; the rest is covered by the independence tests


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


_members = {}


def member(n, idx):
    """Member `idx` of every ensemble of size-n worlds: (partitioned particles, M).  idx 1 has no sources, idx 2 only
    sources; every fifth one is a MakeGalaxies world (its massless share is drawn per seed), the others synthetic with a
    massive fraction that moves with idx -- so the members of an ensemble differ in M."""
    if (n, idx) not in _members:
        if idx == 1:
            part, m = synth(n, frac_massive=0.0, seed=1000 + idx)
        elif idx == 2:
            part, m = synth(n, frac_massive=1.1, seed=1000 + idx)
        elif idx % 5 == 0 and n >= 200:     # MakeGalaxies needs 100 particles per galaxy
            part, m = ob.partition(nb.make_galaxies(n, 2, seed=17 + idx, own_rng=True))
        else:
            part, m = synth(n, frac_massive=0.15 + 0.7 * ((idx * 37) % 100) / 100.0, seed=1000 + idx)
        _members[(n, idx)] = (part, int(m))
    return _members[(n, idx)]


def pinned(n):
    """the knobs that pin a single pipeline to the ensemble's summation order (ISSUE contract)"""
    if n <= 512:
        return dict(matched_shape(n), fused_chain=0, graph=0)
    b = nb.SimBatch(n, [0])
    knobs = b.pinned_knobs()
    b.close()
    assert set(knobs) == {"lanes", "w", "fused_chain"}
    return dict(knobs, graph=0)


_alone = {}


def alone(n, idx, calls):
    """member idx in its own pinned SimPipeline through `calls` = ((steps, dt), ...)"""
    key = (n, idx, tuple(calls))
    if key not in _alone:
        part, m = member(n, idx)
        sim = nb.SimPipeline(n, m)
        sim.configure(**pinned(n))
        sim.set_data(part)
        for steps, dt in calls:
            sim.update(steps, dt)
        _alone[key] = sim.get_data()
        sim.close()
    return _alone[key]


def ensemble(n, idxs):
    parts = np.stack([member(n, i)[0] for i in idxs])
    ms = [member(n, i)[1] for i in idxs]
    b = nb.SimBatch(n, ms)
    b.set_data(parts)
    return b, parts, ms


def checked(count):
    if count <= 64:
        return list(range(count))
    rng = np.random.default_rng(300)
    return sorted({0, count - 1} | set(int(x) for x in rng.choice(np.arange(1, count - 1), CHECKED_OF_300, replace=False)))


@pytest.mark.parametrize("count", [1, 3, 64, 300])
@pytest.mark.parametrize("n", CHAIN_N + LANES_N)
def test_every_member_equals_its_own_pinned_pipeline(n, count):
    idxs = list(range(count))
    b, parts, ms = ensemble(n, idxs)
    if count >= 3:
        assert ms[1] == 0 and ms[2] == n and (len(set(ms)) >= 3 or n < 64)
    shape = b.launch_shape()
    assert shape["path"] == ("chain" if n <= 512 else "lanes")
    b.update(3, DT)
    got = b.get_data()
    b.close()
    assert got.shape == parts.shape
    for i in checked(count):
        want = alone(n, idxs[i], ((3, DT),))
        assert got[i].tobytes() == want.tobytes(), (n, count, i, ms[i], int((got[i] != want).sum()))
    assert not np.array_equal(got[0, :, 0:2], parts[0, :, 0:2])       # it did move


@pytest.mark.parametrize("n", [250, 512, 800, 2000])
def test_call_cutting_changes_no_bit(n):
    """(1, 1, 5, 32, 100) steps in five calls == one 139-step call == the single pipelines in one call."""
    idxs = [0, 1, 2, 3, 5]
    cut, _, _ = ensemble(n, idxs)
    for steps in (1, 1, 5, 32, 100):
        cut.update(steps, DT)
    whole, _, _ = ensemble(n, idxs)
    whole.update(139, DT)
    a, w = cut.get_data(), whole.get_data()
    cut.close()
    whole.close()
    assert a.tobytes() == w.tobytes()
    for i, idx in enumerate(idxs):
        assert a[i].tobytes() == alone(n, idx, ((139, DT),)).tobytes(), (n, idx)
        assert a[i].tobytes() == alone(n, idx, ((1, DT), (1, DT), (5, DT), (32, DT), (100, DT))).tobytes(), (n, idx)


@pytest.mark.parametrize("n", [129, 1000])
def test_every_member_steps_by_its_own_dt(n):
    idxs = list(range(7))
    dts1 = np.array([0.01, 0.02, 0.005, 0.01, 0.04, 0.0025, 0.03], dtype=np.float32)
    dts2 = dts1[::-1].copy()
    b, _, _ = ensemble(n, idxs)
    b.update(4, dts1)
    first = b.get_data()
    assert b.dt_uploads() == 1
    b.update(2, dts1)                    # unchanged step sizes: nothing is uploaded
    assert b.dt_uploads() == 1
    b.step_async(3, dts2)
    b.sync()
    assert b.dt_uploads() == 2
    second = b.get_data()
    b.update(1, 0.02)                    # one dt for all after per-member ones
    assert b.dt_uploads() == 3
    third = b.get_data()
    b.close()
    for i, idx in enumerate(idxs):
        d1, d2 = float(dts1[i]), float(dts2[i])
        assert first[i].tobytes() == alone(n, idx, ((4, d1),)).tobytes(), (n, idx)
        assert second[i].tobytes() == alone(n, idx, ((4, d1), (2, d1), (3, d2))).tobytes(), (n, idx)
        assert third[i].tobytes() == alone(n, idx, ((4, d1), (2, d1), (3, d2), (1, 0.02))).tobytes(), (n, idx)


@pytest.mark.parametrize("n", [250, 800])
def test_members_are_independent_of_each_other_and_of_their_index(n):
    count, j = 300, 137
    idxs = list(range(count))
    b, parts, ms = ensemble(n, idxs)
    b.update(5, DT)
    base = b.get_data()
    b.close()
    # another world in slot j (other particles, another M): no bit of any other member moves
    other, m_other = member(n, 1000)
    assert m_other != ms[j]
    parts2, ms2 = parts.copy(), list(ms)
    parts2[j], ms2[j] = other, m_other
    b = nb.SimBatch(n, ms2)
    b.set_data(parts2)
    b.update(5, DT)
    swapped = b.get_data()
    b.close()
    keep = np.arange(count) != j
    assert swapped[keep].tobytes() == base[keep].tobytes()
    assert swapped[j].tobytes() == alone(n, 1000, ((5, DT),)).tobytes()
    # the same member at index 0 of B = 1 and at index 299 of B = 300
    one, _, _ = ensemble(n, [299])
    one.update(5, DT)
    solo = one.get_member(0)
    one.close()
    assert solo.tobytes() == base[299].tobytes()


def test_golden_fixtures_as_members(golden, manifest):
    """ic_333 (chain path) and ic_1024 (lane-split path) as members beside other worlds, against the reference AVX
    fixtures with the existing one-step / multi-step checkers and their tolerances."""
    for n, slot in ((333, 2), (1024, 0)):
        part, m = ob.partition(golden(f"ic_{n}.bin"))
        e = manifest["sets"][str(n)]["steps"]
        parts = np.stack([synth(n, seed=s)[0] for s in (1, 2, 3)])
        ms = [synth(n, seed=s)[1] for s in (1, 2, 3)]
        parts[slot], ms[slot] = part, m

        def stepped(steps, dt):
            b = nb.SimBatch(n, ms)
            b.set_data(parts)
            b.update(steps, dt)
            out = b.get_member(slot)
            b.close()
            return out

        want1 = golden(e["s1_dt0.01"]["file"]) if "s1_dt0.01" in e else None
        check_one_step(stepped(1, 0.01), part, m, 0.01, want1)
        for key, steps, dt in (("s10_dt0.01", 10, 0.01), ("s3_dt0.05", 3, 0.05)):
            if key not in e:
                continue
            want = golden(e[key]["file"]).astype(np.float64)
            got = stepped(steps, dt).astype(np.float64)
            assert np.linalg.norm(got[:, 0:2] - want[:, 0:2]) / np.linalg.norm(want[:, 0:2]) <= 1e-6
            assert rel_displacement(got, want, part) <= DISPLACEMENT_TOL, (n, key)


@pytest.mark.parametrize("n", [250, 1000])
def test_get_member_and_world_batch_agree_with_get_data(n):
    idxs = [0, 1, 2, 3, 4, 5]
    b, parts, ms = ensemble(n, idxs)
    for i in range(len(idxs)):
        assert b.get_member(i).tobytes() == parts[i].tobytes()        # before any step: what was uploaded
    b.update(6, DT)
    got = b.get_data()
    for i in (5, 0, 3):
        assert b.get_member(i).tobytes() == got[i].tobytes()
    b.close()
    # WorldBatch partitions every member itself: hand it the members in scrambled order
    rng = np.random.default_rng(n)
    raw = np.stack([p[rng.permutation(n)] for p in parts])
    wb = nb.WorldBatch(raw)
    start = wb.particles()
    for i in range(len(idxs)):
        w = nb.World(raw[i])
        assert start[i].tobytes() == w.particles().tobytes()
        w.close()
    sb = nb.SimBatch(n, [int((p[:, 6] > 0).sum()) for p in start])
    sb.set_data(start)
    wb.update_gpu(DT, 0)
    assert wb.particles().tobytes() == start.tobytes()
    wb.update_gpu(DT, 4)
    sb.update(4, DT)
    assert wb.particles().tobytes() == sb.get_data().tobytes()
    dts = np.linspace(0.005, 0.02, len(idxs)).astype(np.float32)
    wb.update_gpu(dts, 3)
    sb.update(3, dts)
    assert wb.member(4).tobytes() == sb.get_member(4).tobytes()
    assert wb.particles().tobytes() == sb.get_data().tobytes()
    wb.close()
    sb.close()


@pytest.mark.parametrize("n", [250, 1000])
def test_a_sim_pipeline_beside_an_ensemble_keeps_its_bits_and_its_state(n):
    """an ensemble shares nothing with a SimPipeline of the same process: bits, graph_stats and launch_shape of a pipeline
    on auto stepped before, between and after ensemble calls equal those of the same pipeline stepped alone"""
    part, m = member(n, 3)

    def walk(with_ensemble):
        out = []
        sim = nb.SimPipeline(n, m)
        sim.set_data(part)
        b = ensemble(n, list(range(9)))[0] if with_ensemble else None
        for steps in (2, 20, 20, 1):
            sim.update(steps, DT)
            out.append((sim.get_data().tobytes(), sim.graph_stats(), sim.launch_shape(), sim.fused_steps()))
            if b:
                b.update(steps + 1, 2 * DT)
        if b:
            for i in range(9):
                assert b.get_member(i).tobytes() == alone(n, i, ((3, 2 * DT), (21, 2 * DT), (21, 2 * DT), (2, 2 * DT))).tobytes()
            b.close()
        sim.update(3, DT)
        out.append((sim.get_data().tobytes(), sim.graph_stats(), sim.launch_shape(), sim.fused_steps()))
        sim.close()
        return out

    assert walk(True) == walk(False)


def test_the_callers_rand_stream_is_left_alone():
    import ctypes as C
    libc = C.CDLL(None)
    libc.srand(4242)
    want = [libc.rand() for _ in range(4)]
    libc.srand(4242)
    b, _, _ = ensemble(64, [0, 3])
    b.update(2, DT)
    b.close()
    assert [libc.rand() for _ in range(4)] == want
