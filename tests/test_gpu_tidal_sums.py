"""The summation scheme of the tidal tensor on the device, held to the checkers tests/test_tidal_cpu.py holds the numpy model to
(needs an MI355X: `pytest -m gpu`; worlds and exact results: tests/tidal_ref.py).  The contract (include/nbody_tidal.h, DESIGN.md
"The tidal tensor"): fp32 sums over blocks of 256 sources, float64 block totals in eight slices of whole blocks, the factor 3
and the difference 3A - D in float64, each component rounded once.

On tidal_ref.exact_world every instruction of the statement is exact (dx = -1, dy = 0, q = 4, u = 1/2), so a result is an
exactly known number rounded as the scheme rounds it:
  exact worlds  one source, or two equal ones, of any mantissa: 0 ulp, on every route -- the test a per-pair fp32 rounding of
                3 * tx ("merged diagonal") fails;
  pattern 1     M equal sources whose G*m has three bits: every block total and every float64 sum is exact, the result is M
                times the single term to the final rounding, <= 1/2 ulp -- every source added exactly once, across the 8-wide
                loop, its tail, the block and the slice ends;
  pattern 2     the witness, one source 2^33 times as heavy as its 65 535 neighbours: within E = 1 ulp -- the test fp32 block
                totals ("f32 totals") fail;
  and the same witness seen by 1, 129 and 1 000 copies of the probe gives the same bytes for every copy.
A map's sample is a pixel centre: the views below put centres exactly on exact_probe() (asserted from tidal_ref.pixel_points)."""
from fractions import Fraction

import numpy as np
import pytest

import nbody_amd as nb
import tidal_ref as tr
from test_gpu_tidal import SOURCES
from test_tidal_cpu import EXACT_MASSES, WITNESS_E, WITNESS_M
from tidal_ref import ulps_off

pytestmark = pytest.mark.gpu

F32 = np.float32
SPLIT, WAVE = 1, 2
SHAPES = {"split": SPLIT, "wave": WAVE}
SOFT = tr.EXACT_SOFT
PROBE = tr.exact_probe()
EQUAL_M = sorted(set(m for m in SOURCES if m > 0) | {8, 9, 511, 512, 513, 2047, 65536})
ENSEMBLE_M = [m for m in EQUAL_M if m <= 2999] + [2999]
WITNESS_AT = (0, 255, 256, 32868, 65535)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def view_on_the_probe(width=1):
    """a width x 1 view whose every centre is exact_probe(): x = ((i + 0.5) - 0.5) / 2^40 + 9 rounds to 9 for every i < 2^16"""
    view = nb.RenderView.make((float(PROBE[0, 0]), float(PROBE[0, 1])), (0.5, 0.5), 2.0 ** 40, width, 1, 1.0)
    assert tr.pixel_points(view).tobytes() == np.repeat(PROBE, width, axis=0).tobytes()
    return view


def pipeline(masses):
    sim = nb.SimPipeline(len(masses), len(masses))
    sim.set_data(tr.exact_world(masses))
    return sim


def pipeline_routes(sim, copies=(1, 130)):
    """(route name, T (3,)) of the four pipeline kernels; with several copies of the probe every copy must agree"""
    for name, shape in SHAPES.items():
        sim.configure(tidal_shape=shape)
        for n in copies:
            at = sim.tidal_at(np.repeat(PROBE, n, axis=0), SOFT)
            img = sim.tidal_map(view_on_the_probe(n), SOFT).reshape(-1, 3)
            for what, got in ((f"tidal_at {name}", at), (f"tidal_map {name}", img)):
                assert got.shape == (n, 3) and got.tobytes() == np.repeat(got[:1], n, axis=0).tobytes(), (what, n, "the copies differ")
                yield f"{what} x {n}", got[0]


def worst_ulps(got, masses):
    return max(ulps_off(g, e) for g, e in zip(got, tr.exact_tensor(masses)))


def member(n, masses):
    """n particles at EXACT_P, the first len(masses) with these masses, the rest massless"""
    a = tr.exact_world(np.concatenate([np.asarray(masses, dtype=F32), np.zeros(n - len(masses), dtype=F32)]))
    assert a.shape[0] == n
    return a


def ensemble_results(uniform_n, mass_lists):
    """(T at the probe, T of the one-pixel map) per member: a uniform ensemble of size uniform_n, or a ragged one (None)"""
    if uniform_n is None:
        b = nb.SimBatch.ragged([len(m) for m in mass_lists], [len(m) for m in mass_lists])
        b.set_data([tr.exact_world(m) for m in mass_lists])
    else:
        b = nb.SimBatch(uniform_n, [len(m) for m in mass_lists])
        b.set_data(np.stack([member(uniform_n, m) for m in mass_lists]))
    at, img = b.tidal_at(np.repeat(PROBE, 130, axis=0), SOFT), b.tidal_map(view_on_the_probe(130), SOFT).reshape(len(mass_lists), -1, 3)
    b.close()
    for got in (at, img):
        assert got.tobytes() == np.repeat(got[:, :1], 130, axis=1).tobytes(), "the copies differ"
    return at[:, 0], img[:, 0]


# ---- the exact worlds --------------------------------------------------------------------------------------------------------------------

def test_the_premise_scaling_the_mass_by_a_power_of_two_scales_t_exactly():
    """... so the statement's products are exact beside u = 1/2, and what is left is the scheme's own rounding"""
    base = None
    for k in (0, -20, 7, 30):
        sim = pipeline([F32(1.2345678) * F32(2.0 ** k)])
        for route, got in pipeline_routes(sim, copies=(1,)):
            assert np.all(np.isfinite(got)) and got[0] < 0 and got[2] < 0
            scaled = np.ldexp(got.astype(np.float64), -k)
            base = scaled if base is None else base
            assert np.array_equal(scaled, base), (route, k, got)
        sim.close()


def test_exact_worlds_are_met_to_the_last_bit_on_every_route():
    """0 ulp: the exact tensor G*m (-1/32, 0, -1/8) is a float32.  "merged diagonal" is 1 ulp off on every one of these worlds
    (tests/test_tidal_cpu.py)."""
    for masses in EXACT_MASSES:
        sim = pipeline(masses)
        for route, got in pipeline_routes(sim):
            assert worst_ulps(got, masses) == 0.0, (route, masses, got)
            assert not got[1:2].view(np.uint32).any(), (route, "xy is not +0")
        sim.close()
    # ensembles: the four worlds as members of a chain-sized and of a lane-split-sized uniform ensemble, and of a ragged one
    for n in (300, 700, None):
        lists = [list(m) for m in EXACT_MASSES] + [[0.5] * 40]
        for got in ensemble_results(n, lists):
            for masses, t in zip(EXACT_MASSES, got):
                assert worst_ulps(t, masses) == 0.0, (n, masses, t)
    print(f"[tidal sums] exact worlds | {len(EXACT_MASSES)} worlds | 0 ulp on tidal_at, tidal_map (both shapes) and the ensembles")


# ---- pattern 1: equal terms --------------------------------------------------------------------------------------------------------------

def equal(m):
    return np.full(m, tr.WITNESS_SMALL, dtype=F32)


@pytest.mark.parametrize("m", EQUAL_M)
def test_equal_sources_are_each_added_exactly_once(m):
    """M times the single-source term, formed in integer arithmetic (tidal_ref.exact_tensor: Fractions), to the final rounding"""
    single = tr.exact_tensor(equal(1))
    assert tr.exact_tensor(equal(m)) == tuple(m * t for t in single) and Fraction(float(F32(m * 10 * tr.WITNESS_SMALL))) == m * Fraction(10, 4096)
    sim = pipeline(equal(m))
    worst = 0.0
    for route, got in pipeline_routes(sim):
        e = worst_ulps(got, equal(m))
        worst = max(worst, e)
        assert e <= 0.5, (route, m, got, e)
    sim.close()
    print(f"[tidal sums] equal sources | M = {m} | worst {worst:.3f} ulp on the four pipeline kernels (1/2 allowed)")


@pytest.mark.parametrize("kind", ["uniform chain-sized", "uniform lane-split-sized", "ragged"])
def test_equal_sources_in_the_ensembles(kind):
    ms = {"uniform chain-sized": [m for m in ENSEMBLE_M if m <= 511], "uniform lane-split-sized": ENSEMBLE_M, "ragged": ENSEMBLE_M}[kind]
    n = {"uniform chain-sized": 511, "uniform lane-split-sized": 2999, "ragged": None}[kind]
    assert min(ms) == 1 and (kind == "uniform chain-sized" or (max(ms) == 2999 and any(m <= 511 for m in ms)))
    worst = 0.0
    for got in ensemble_results(n, [equal(m) for m in ms]):
        for m, t in zip(ms, got):
            e = worst_ulps(t, equal(m))
            worst = max(worst, e)
            assert e <= 0.5, (kind, m, t, e)
    print(f"[tidal sums] equal sources | {kind} ensemble, M in {ms} | worst {worst:.3f} ulp (1/2 allowed)")


# ---- pattern 2: the witness ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("at", WITNESS_AT)
def test_the_witness_is_within_one_ulp(at):
    """E = 1 ulp (tests/test_tidal_cpu.py derives it and its model meets it): the big term's block loses its 255 neighbours, at
    most half an ulp, every other block total reaches the float64 sums whole, and the final rounding costs half an ulp.  fp32
    totals are more than 2 E off."""
    masses = tr.witness_masses(WITNESS_M, at)
    sim = pipeline(masses)
    worst = 0.0
    for route, got in pipeline_routes(sim):
        e = worst_ulps(got, masses)
        worst = max(worst, e)
        assert e <= WITNESS_E, (route, at, got, e)
    sim.close()
    print(f"[tidal sums] witness | M = {WITNESS_M}, the big source at {at} | worst {worst:.3f} ulp on the four pipeline kernels (E = {WITNESS_E})")


@pytest.mark.parametrize("n", [2999, None], ids=["uniform", "ragged"])
def test_the_witness_bound_in_the_ensembles(n):
    """M = 2 999 is twelve blocks, two per slice at most: fp32 totals would stay inside E here too, so this run holds the
    bound and has no teeth against that defect (tests/test_gpu_sums.py says the same of its ensembles)."""
    lists = [tr.witness_masses(2999, at) for at in (0, 255, 256, 2998)] + [equal(300)]
    for got in ensemble_results(n, lists):
        for masses, t in zip(lists[:-1], got):
            assert worst_ulps(t, masses) <= WITNESS_E, (n, t)


# ---- independence of the launch --------------------------------------------------------------------------------------------------------------

def test_the_witness_seen_by_1_129_and_1000_copies_of_the_probe_gives_the_same_bytes():
    masses = tr.witness_masses(WITNESS_M, 32868)
    sim = pipeline(masses)
    results = {route: got.tobytes() for route, got in pipeline_routes(sim, copies=(1, 129, 1000))}
    sim.close()
    assert len(results) == 12 and len(set(results.values())) == 1, {k: np.frombuffer(v, dtype=F32) for k, v in results.items()}
