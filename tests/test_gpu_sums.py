"""The summation scheme of the force, field and energy kernels, pinned on worlds whose sums are known exactly (needs an MI355X:
`pytest -m gpu`; helper and reasoning: tests/sum_witness.py; the checker's teeth, without a GPU: tests/test_sum_witness_cpu.py).

Every source of a witness world sits at one point with a power-of-two mass, every tracer at a power-of-two offset: the term of
one source is measured from a world with ONE source (bit for bit, anchored to the float64 formula by check_one_step), scaling
the mass by 2^k scales it exactly (asserted), and the sum of M terms is then formed in integer arithmetic.  Three patterns:

  1  M equal terms: |acc - M t| < t / 4 -- no source missing, none added twice, whichever index it has;
  2  one term 2^33 (2^32 for the lane-split kernel) times the others, so that one block of small terms is a quarter ulp of
     the big one: within E(shape) ulps of the exact sum, E = 1 + 1/2 per plain addition that joins partial sums (DESIGN.md
     section 5 "Summation, per kernel family").  Cases marked `teeth` in sum_witness.CASES are those at which the same blocks
     with plain totals, or one plain running sum, provably leave E (15 and 58 ulps at 16 384 and 65 536 sources on one wave);
  3  mirrored: +big, the smalls, -big from the mirror point: the exact sum is the smalls alone, the bound is in ulps of big.

The one-workgroup chain and the ensembles hold at most 3 000 particles: twelve blocks of 256 give the compensation no teeth
there, so they run pattern 1 at every block, tile and granule edge and pattern 2 for the bound only.  An ensemble member is at
most 3 000 particles INCLUDING its tracers, so its largest source count beside one tracer is 2 999 (511 on the chain path).

Every case prints its signed error in ulps and its bound (`pytest -rP`); profiles/r14_sum_witness.txt is one run's table."""
from fractions import Fraction

import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
import sum_witness as sw
from gpu_common import check_one_step, run
from test_gpu_field import SOURCES as FIELD_SOURCES
from test_gpu_parity import GRANULE_COUNTS, GRANULE_KNOBS, SWEEP_COUNTS, SWEEP_KNOBS

pytestmark = pytest.mark.gpu

F32 = np.float32
DT = 0.01
SMALL = F32(sw.M_SMALL)
TRACERS = 3 * sw.PER_POSITION
WHERE = sw.tracer_positions(TRACERS, 3)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def big(L):
    return F32(SMALL * F32(2.0 ** sw.big_shift(L)))


def launch(part, m, steps=1, **knobs):
    sim = nb.SimPipeline(part.shape[0], m)
    sim.configure(**knobs)
    sim.set_data(part)
    sim.update(steps, DT)
    shape, out = sim.launch_shape(), sim.get_data()
    sim.close()
    return out, shape


# ---- the measured terms ------------------------------------------------------------------------------------------------------

_TERMS = {}


def step_terms(mass, positions=(0, 1, 2), src=sw.P0):
    """acc of a tracer at each position in a world with ONE source of this mass: the term itself, (len(positions), 2) float32"""
    key = (float(mass), tuple(positions), tuple(src))
    if key not in _TERMS:
        part = sw.world([mass], positions=positions, tracers=3 * len(positions), src_pos=[src])
        got = run(part, 1, 1, DT, k=1, w=1, lanes=1)
        check_one_step(got, part, 1, DT)          # the anchor: the term is the float64 formula's, within the stated tolerance
        rows = sw.distinct(got[1:, 4:6], sw.tracer_positions(3 * len(positions), len(positions)))
        assert len(rows) == len(positions), "tracers at one position differ"
        _TERMS[key] = np.stack([row for _, row in rows])
    return _TERMS[key]


def field_terms(mass):
    """(Phi, g) of one source of this mass at the three tracer points: (3,) and (3, 2) float32"""
    key = ("field", float(mass))
    if key not in _TERMS:
        sim = nb.SimPipeline(1 + TRACERS, 1)
        sim.set_data(sw.world([mass]))
        pts = np.asarray([sw.tracer_point(p) for p in range(3)], dtype=F32)
        phi, g = sim.potential_at(pts, sw.TRACER_RADIUS), sim.acceleration_at(pts, sw.TRACER_RADIUS)
        per_particle = sim.potential()[1:]
        sim.close()
        # anchors: g is the step kernels' statement with the softening as the radius; Phi against the float64 formula
        assert np.array_equal(g, step_terms(mass))
        d2 = np.asarray([o[0] ** 2 + o[1] ** 2 + sw.TRACER_RADIUS for o in sw.OFFSETS], dtype=np.float64)
        want = -float(F32(nb.NB_G) * F32(mass)) / np.sqrt(d2)
        assert np.all(np.abs(phi - want) <= 1e-5 * np.abs(want))
        assert np.array_equal(per_particle, phi[WHERE])      # a tracer's Phi_i is the probe's
        _TERMS[key] = (phi, g)
    return _TERMS[key]


def test_the_premise_scaling_a_mass_by_a_power_of_two_scales_the_term_exactly():
    ts = step_terms(SMALL)
    assert np.all((ts != 0) == (np.asarray(sw.OFFSETS) != 0))
    for L in (sw.L_LANE, sw.L_CLASSIC):
        assert np.array_equal(step_terms(big(L)), ts * F32(2.0 ** sw.big_shift(L)))
        assert np.array_equal(field_terms(big(L))[0], field_terms(SMALL)[0] * F32(2.0 ** sw.big_shift(L)))
    pos = (sw.MIRROR_POSITION,)
    assert np.array_equal(step_terms(big(sw.L_CLASSIC), pos, sw.mirror_point()), -step_terms(big(sw.L_CLASSIC), pos))
    assert np.array_equal(step_terms(SMALL, pos), ts[sw.MIRROR_POSITION:sw.MIRROR_POSITION + 1])


# ---- checking -----------------------------------------------------------------------------------------------------------------

def check(label, values, where, exact, bound, scale=None, identical=True):
    """values: one row per tracer; where: its position index; exact[p][component]: Fractions.  Prints every distinct result's
    signed error in ulps, then asserts |error| <= bound."""
    values = np.asarray(values).reshape(len(where), -1)
    rows = sw.distinct(values, where)
    if identical:
        assert len(rows) == len(np.unique(where)), f"{label}: tracers at one position differ"
    bad = []
    for p, row in rows:
        for comp, got in enumerate(row):
            e = sw.err_ulps(got, exact[p][comp], None if scale is None else scale[p][comp])
            line = f"[sum] {label} | position {p} component {comp} | {e:+.3f} ulp | E = {bound}"
            print(line)
            if not abs(e) <= bound:
                bad.append(line)
    assert not bad, bad


def exact_big(m, small, large):
    """(m - 1) small terms and one big one, per position and component"""
    small, large = np.asarray(small).reshape(len(small), -1), np.asarray(large).reshape(len(large), -1)
    return [[sw.exact_sum([(m - 1, s), (1, b)]) for s, b in zip(rs, rb)] for rs, rb in zip(small, large)]


def check_once(label, values, where, terms, m):
    """pattern 1: |value - m t| < |t| / 4 for every tracer and component, and an exact zero where the term is zero"""
    values = np.asarray(values, dtype=np.float64).reshape(len(where), -1)
    t = np.asarray(terms, dtype=np.float64).reshape(len(terms), -1)[where]
    d = np.abs(values - m * t)                # exact: m < 2^13, t and the value are float32 of neighbouring binades
    ok = np.where(t == 0, values == 0, d < np.abs(t) / 4)
    assert np.all(ok), f"{label}: {m} sources, worst |acc - M t| = {np.max(d[t != 0] / np.abs(t[t != 0])):.3f} t"
    return float(np.max(d[t != 0] / np.abs(t[t != 0]))) if np.any(t != 0) else 0.0


def big_world(c):
    """the world of pattern-2 or pattern-3 case c: (particles, tracer positions, exact sums, scale of the ulp)"""
    L, m = sw.case_L(c), c["m"]
    if c["pattern"] == "mirrored":
        pos = (sw.MIRROR_POSITION,)
        ts, tb = step_terms(SMALL, pos), step_terms(big(L), pos)
        return (sw.mirrored(m, L), np.zeros(TRACERS, dtype=int), [[sw.exact_sum([(m - 2, t)]) for t in ts[0]]],
                [[Fraction(float(t)) for t in tb[0]]])
    part = sw.world(sw.one_big(m, L, sw.big_positions(m, L)[c["at"]]))
    return part, WHERE, exact_big(m, step_terms(SMALL), step_terms(big(L))), None


def name(c):
    return f"{c['pattern']}-{c['at']}-M{c['m']}" + "".join(f"-{k}{v}" for k, v in c["shape"].items()) + ("-teeth" if c["teeth"] else "")


def of(family):
    return [c for c in sw.CASES if c["family"] == family]


# ---- the classic step kernel ------------------------------------------------------------------------------------------------

# both source routes and k = 1, 2; the 65 536-source case once per route
CLASSIC = [(c, k, v) for c in of("classic") for k in (1, 2) for v in (0, 1) if c["m"] <= 16384 or k == 1]


@pytest.mark.parametrize("c,k,variant", CLASSIC, ids=[f"{name(c)}-k{k}-variant{v}" for c, k, v in CLASSIC])
def test_classic_kernel_sums_within_E(c, k, variant):
    part, where, exact, scale = big_world(c)
    s = c["shape"]
    got = run(part, c["m"], 1, DT, lanes=1, variant=variant, k=k, w=s["w"], split=s.get("split", 1), passes=s.get("passes", 1))
    check(f"classic {name(c)} k={k} variant={variant}", got[c["m"]:, 4:6], where, exact, sw.case_E(c), scale)


@pytest.mark.parametrize("split", [3, 16])
def test_classic_kernel_fused_finish_and_graph_chain_within_E(split):
    """The parts added by the tile's last workgroup instead of finish_kernel: the same bound, and the same bits.  A hipGraph
    chain of two steps equals two plain launches bitwise; its first step is the plain launch checked here."""
    c = sw.case("classic", 16384, False, at="middle", w=4, split=split)
    part, where, exact, _ = big_world(c)
    knobs = dict(lanes=1, variant=1, k=2, w=4, split=split)
    outs = []
    for fused in (0, 1):
        outs.append(run(part, c["m"], 1, DT, fused_finish=fused, **knobs))
        check(f"classic {name(c)} fused_finish={fused}", outs[-1][c["m"]:, 4:6], where, exact, sw.case_E(c))
        assert run(part, c["m"], 2, DT, fused_finish=fused, graph=1, **knobs).tobytes() == \
            run(part, c["m"], 2, DT, fused_finish=fused, graph=0, **knobs).tobytes()
    assert outs[0].tobytes() == outs[1].tobytes()


# ---- pattern 1 on the classic kernel: every source exactly once --------------------------------------------------------------

@pytest.mark.parametrize("knobs", SWEEP_KNOBS, ids=[str(k) for k in SWEEP_KNOBS])
def test_exactly_once_at_the_source_counts_of_the_route_sweep(knobs):
    ts, worst = step_terms(SMALL), 0.0
    for m in SWEEP_COUNTS:
        part = sw.world(sw.equal_masses(m))
        for variant, unit in ((0, 64), (1, 64)):
            got = run(part, m, 1, DT, lanes=1, variant=variant, unit=unit, **knobs)
            worst = max(worst, check_once(f"{knobs} variant {variant}", got[m:, 4:6], WHERE, ts, m))
    print(f"[sum] exactly once, route sweep {knobs} | {len(SWEEP_COUNTS)} counts x 2 routes | worst |acc - M t| = {worst:.4f} t | bound 0.25 t")


@pytest.mark.parametrize("unit", [8, 16, 32, 64])
def test_exactly_once_at_the_source_counts_of_the_fine_granules(unit):
    ts, worst = step_terms(SMALL), 0.0
    for m in GRANULE_COUNTS:
        part = sw.world(sw.equal_masses(m))
        for knobs in GRANULE_KNOBS:
            got = run(part, m, 1, DT, lanes=1, unit=unit, **knobs)
            worst = max(worst, check_once(f"{knobs} unit {unit}", got[m:, 4:6], WHERE, ts, m))
    print(f"[sum] exactly once, unit {unit} | {len(GRANULE_COUNTS)} counts x {len(GRANULE_KNOBS)} shapes | worst |acc - M t| = {worst:.4f} t | bound 0.25 t")


# ---- the lane-split kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", of("lane"), ids=name)
def test_lane_split_kernel_sums_within_E(c):
    part, where, exact, _ = big_world(c)
    got, shape = launch(part, c["m"], lanes=c["shape"]["lanes"], w=c["shape"]["w"])
    assert shape["lanes"] == c["shape"]["lanes"] and shape["w"] == c["shape"]["w"]
    check(f"lane-split {name(c)}", got[c["m"]:, 4:6], where, exact, sw.case_E(c))


# ---- the sharded step --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", of("sharded"), ids=name)
def test_sharded_step_sums_within_E(c):
    """One wave per receiver tile over the gathered sources (padded slices), and the overlapped step's two launches: own slice,
    then the rest as two ranges.  A tracer's order depends on the rank that owns it, so tracers at one position may differ."""
    part, where, exact, _ = big_world(c)
    g = nb.LocalShardGroup(part.shape[0], c["m"], c["shape"]["ranks"], overlap=c["shape"]["overlap"], k=1, w=1)
    g.set_data(part)
    g.step(1, DT)
    got = g.get_data(0)
    g.close()
    check(f"sharded {name(c)}", got[c["m"]:, 4:6], where, exact, sw.case_E(c), identical=False)


def test_sharded_step_adds_every_source_exactly_once():
    ts = step_terms(SMALL)
    for m in (63, 64, 65, 257, 1031, 2111):
        part = sw.world(sw.equal_masses(m))
        for ranks, overlap in ((2, 0), (2, 1), (3, 0), (3, 1)):
            g = nb.LocalShardGroup(part.shape[0], m, ranks, overlap=overlap)
            g.set_data(part)
            g.step(1, DT)
            got = g.get_data(ranks - 1)
            g.close()
            check_once(f"sharded P={ranks} overlap={overlap}", got[m:, 4:6], WHERE, ts, m)


# ---- the one-workgroup chain and the ensembles --------------------------------------------------------------------------------

ENSEMBLE_POSITIONS = (2, 0, 1)      # a member with one tracer has it where both components are non-zero


def member(m, n, masses=None):
    return sw.world(sw.equal_masses(m) if masses is None else masses, positions=ENSEMBLE_POSITIONS, tracers=n - m)


def check_member(label, got, m, n):
    return check_once(label, got[m:, 4:6], sw.tracer_positions(n - m, 3), step_terms(SMALL, ENSEMBLE_POSITIONS), m)


@pytest.mark.parametrize("n,pairs", [(512, [(1, 63), (64, 65), (255, 256), (257, 511)]), (1300, [(513, 1000)]), (3000, [(1000, 2999)])])
def test_uniform_ensembles_add_every_source_exactly_once(n, pairs):
    """N <= 512: batch_chain_kernel (chain_body, the one-workgroup chain); above: batch_lane_split_kernel<8, 8> / <16, 4>; the
    members found by block index (BatchParams)."""
    worst = 0.0
    for ms in pairs:
        b = nb.SimBatch(n, list(ms))
        b.set_data(np.stack([member(m, n) for m in ms]))
        b.update(1, DT)
        got = b.get_data()
        b.close()
        for i, m in enumerate(ms):
            worst = max(worst, check_member(f"ensemble N={n} member {i}", got[i], m, n))
    print(f"[sum] exactly once, uniform ensemble N = {n}, M in {pairs} | worst |acc - M t| = {worst:.4f} t | bound 0.25 t")


def test_a_ragged_ensemble_adds_every_source_exactly_once():
    """the same three kernels, the members found through the lists (RaggedParams)"""
    sizes = [(63, 100), (257, 300), (511, 512), (513, 600), (1000, 1300), (2999, 3000)]
    r = nb.SimBatch.ragged([n for _, n in sizes], [m for m, _ in sizes])
    r.set_data([member(m, n) for m, n in sizes])
    r.update(1, DT)
    got = r.get_data()
    r.close()
    worst = max(check_member(f"ragged member {i}", got[i], m, n) for i, (m, n) in enumerate(sizes))
    print(f"[sum] exactly once, ragged ensemble (M, N) = {sizes} | worst |acc - M t| = {worst:.4f} t | bound 0.25 t")


@pytest.mark.parametrize("m,n,L,shape", [(511, 512, sw.L_CLASSIC, dict(w=4)), (2999, 3000, sw.L_LANE, dict(w=16, lanes=4))],
                         ids=["chain-N512", "lane-split-N3000"])
def test_ensembles_stay_within_E_with_one_big_term(m, n, L, shape):
    """Bound only: twelve blocks at the most give the compensation no teeth here (tests/test_sum_witness_cpu.py)."""
    at = sw.big_positions(m, L)["middle"]
    b = nb.SimBatch(n, [m])
    b.set_data(member(m, n, sw.one_big(m, L, at))[None])
    b.update(1, DT)
    got = b.get_data()[0]
    b.close()
    exact = exact_big(m, step_terms(SMALL, ENSEMBLE_POSITIONS), step_terms(big(L), ENSEMBLE_POSITIONS))
    check(f"ensemble N={n} M={m} big at {at} {shape}", got[m:, 4:6], sw.tracer_positions(n - m, 3), exact, sw.E(**shape))


# ---- the field sampler -------------------------------------------------------------------------------------------------------

PROBES = np.asarray([sw.tracer_point(p) for p in range(3)], dtype=F32)[WHERE]


def sample(part, m, shape):
    sim = nb.SimPipeline(part.shape[0], m)
    sim.configure(field_shape=shape, gravity_shape=shape)
    sim.set_data(part)
    phi, g = sim.potential_at(PROBES, sw.TRACER_RADIUS), sim.acceleration_at(PROBES, sw.TRACER_RADIUS)
    sim.close()
    return phi, g


@pytest.mark.parametrize("shape", [1, 2], ids=["split", "wave"])
def test_field_sampler_adds_every_source_exactly_once(shape):
    tphi, tg = field_terms(SMALL)
    worst = 0.0
    for m in FIELD_SOURCES:
        phi, g = sample(sw.world(sw.equal_masses(m)) if m else sw.world([]), m, shape)
        if m == 0:
            assert np.all(phi == 0) and np.all(g == 0)
            continue
        worst = max(worst, check_once(f"Phi shape {shape}", phi, WHERE, tphi, m), check_once(f"g shape {shape}", g, WHERE, tg, m))
    print(f"[sum] exactly once, field sampler shape {shape}, M in {FIELD_SOURCES} | worst |value - M t| = {worst:.4f} t | bound 0.25 t")


@pytest.mark.parametrize("shape", [1, 2], ids=["split", "wave"])
@pytest.mark.parametrize("c", of("field"), ids=name)
def test_field_sampler_sums_within_one_ulp(c, shape):
    """fp32 over blocks of 256 sources, float64 block totals in eight slices, one rounding to float32: Phi within 1 ulp, g
    within E = 1 ulp.  Float32 block totals leave both (tests/test_sum_witness_cpu.py)."""
    m, L = c["m"], sw.L_FIELD
    phi, g = sample(sw.world(sw.one_big(m, L, sw.big_positions(m, L)[c["at"]])), m, shape)
    (sphi, sg), (bphi, bg) = field_terms(SMALL), field_terms(big(L))
    check(f"field Phi {name(c)} shape={shape}", phi, WHERE, exact_big(m, sphi, bphi), 1.0)
    check(f"field g {name(c)} shape={shape}", g, WHERE, exact_big(m, sg, bg), sw.E_FIELD)


# ---- the diagnostics ---------------------------------------------------------------------------------------------------------

def source_phi_term(mass):
    """-Phi_0 of a world of two coincident sources (SMALL, mass): the term G m / sqrt(0 + 1) of the second on the first"""
    key = ("source", float(mass))
    if key not in _TERMS:
        sim = nb.SimPipeline(2 + TRACERS, 2)
        sim.set_data(sw.world([SMALL, mass]))
        _TERMS[key] = float(-sim.potential()[0])
        sim.close()
        want = float(F32(nb.NB_G) * F32(mass))                         # the anchor; equal when rsq(1) = 1 exactly
        assert abs(_TERMS[key] - want) <= 1e-5 * want
    return _TERMS[key]


def energy_exact_and_bound(masses):
    """energy()["potential"] = 1/2 sum_i m_i Phi_i over the sources of a witness world, exactly, and the bound: what the
    documented scheme (fp32 blocks, float64 totals: sum_witness.field_model) loses inside its blocks, plus 2^-52 relative."""
    masses = np.asarray(masses, dtype=F32)
    m = masses.size
    kinds = np.unique(masses)
    x = np.asarray([source_phi_term(v) for v in kinds], dtype=F32)[np.searchsorted(kinds, masses)]
    total = sum(int(n) * Fraction(float(v)) for v, n in zip(*np.unique(x, return_counts=True)))
    # per receiver i: the sum over j != i.  Receivers of one mass outside the big term's block all see the same sum.
    heavy = int(np.argmax(masses))
    block = range(heavy // sw.L_FIELD * sw.L_FIELD, min((heavy // sw.L_FIELD + 1) * sw.L_FIELD, m)) if masses[heavy] != masses.min() else range(0)
    inside = set(block)
    outside = next((i for i in range(m) if i not in inside), None)

    def modelled(i):
        xi = x.copy()
        xi[i] = 0.0                       # the masked pair adds nothing
        return Fraction(float(sw.field_model(xi, "f64")))
    shared = modelled(outside) if outside is not None else None
    model = exact = Fraction(0)
    for i in range(m):
        mi, xi = Fraction(float(masses[i])), Fraction(float(x[i]))
        exact -= mi * (total - xi)
        model -= mi * (modelled(i) if i in inside else shared)
    exact, model = exact / 2, model / 2
    return exact, abs(model - exact) + abs(exact) * Fraction(1, 2 ** 52)


@pytest.mark.parametrize("m", [c for c in FIELD_SOURCES if c > 1])
def test_diagnostics_with_equal_sources(m):
    """M coincident sources of one power-of-two mass: Phi_i of a source is -(M - 1) terms and Phi of a tracer -M terms, both
    under the exactly-once condition; the potential energy is -M (M - 1) m G m / 2 within what the documented scheme loses
    inside its float32 blocks -- nothing, when the term G m / sqrt(1) is G m itself -- plus 2^-52 relative."""
    part = sw.world(sw.equal_masses(m))
    sim = nb.SimPipeline(part.shape[0], m)
    sim.set_data(part)
    phi, e = sim.potential(), sim.energy()["potential"]
    sim.close()
    g = source_phi_term(SMALL)
    assert np.all(np.abs(phi[:m].astype(np.float64) + (m - 1) * g) < g / 4)
    check_once("potential()", phi[m:], WHERE, field_terms(SMALL)[0], m)
    exact, bound = energy_exact_and_bound(sw.equal_masses(m))
    err = Fraction(e) - exact
    print(f"[sum] diagnostics, {m} equal sources | energy()['potential'] error {float(err / abs(exact)):+.3e} relative | bound {float(bound / abs(exact)):.3e}")
    assert abs(err) <= bound


@pytest.mark.parametrize("c", of("diag"), ids=name)
def test_diagnostics_sums_with_one_big_term(c):
    m, L = c["m"], sw.L_FIELD
    masses = sw.one_big(m, L, sw.big_positions(m, L)[c["at"]])
    part = sw.world(masses)
    sim = nb.SimPipeline(part.shape[0], m)
    sim.set_data(part)
    phi, e = sim.potential(), sim.energy()["potential"]
    sim.close()
    check(f"potential() {name(c)}", phi[m:], WHERE, exact_big(m, field_terms(SMALL)[0], field_terms(big(L))[0]), 1.0)
    exact, bound = energy_exact_and_bound(masses)
    err = Fraction(e) - exact
    print(f"[sum] energy()['potential'] {name(c)} | error {float(err / abs(exact)):+.3e} relative | bound {float(bound / abs(exact)):.3e}")
    assert abs(err) <= bound


@pytest.mark.parametrize("at", ["equal", "first", "middle"])
def test_ensemble_energy_of_one_member(at):
    m, n, L = 2999, 3000, sw.L_FIELD
    masses = sw.equal_masses(m) if at == "equal" else sw.one_big(m, L, sw.big_positions(m, L)[at])
    b = nb.SimBatch(n, [m])
    b.set_data(member(m, n, masses)[None])
    e = b.energy()[0]["potential"]
    b.close()
    exact, bound = energy_exact_and_bound(masses)
    err = Fraction(e) - exact
    print(f"[sum] SimBatch energy()['potential'] M={m} big {at} | error {float(err / abs(exact)):+.3e} relative | bound {float(bound / abs(exact)):.3e}")
    assert abs(err) <= bound


# ---- one measured comparison against the reference's summation order ----------------------------------------------------------

def test_a_clustered_world_is_no_further_from_float64_than_the_avx_order():
    """65 536 sources in a cluster ten sigma away from 128 tracers, masses in [1, 2] x 100: the pulls align, which is where a
    sequential fp32 sum drifts.  rms over the tracers of |acc - acc_f64| / sum|contribution|, GPU <= the reference's AVX order
    on the same input (closer to float64 than the AVX path is acceptable).  No ratio is asserted."""
    rng = np.random.default_rng(14)
    m, tracers, sigma = 65536, 128, 100.0
    a = np.zeros((m + tracers, 8), dtype=F32)
    a[:m, 0:2] = rng.standard_normal((m, 2)) * sigma
    a[:m, 6] = 100.0 * (1.0 + rng.random(m))
    a[:m, 7] = 1.0
    a[m:, 0:2] = np.asarray([10.0 * sigma, 0.0]) + rng.standard_normal((tracers, 2)) * 0.1 * sigma
    a[m:, 7] = 0.5
    idx = np.arange(m, m + tracers)
    acc64, mag = ob.acc_f64_subset(a, m, idx)

    def rms(acc):
        return float(np.sqrt(np.mean(((acc.astype(np.float64) - acc64) / mag) ** 2)))
    avx = rms(ob.acc_avx_subset(a, m, idx))
    for label, knobs in (("default shape", dict()), ("w = 1", dict(k=1, w=1))):
        got, shape = launch(a, m, **knobs)
        gpu = rms(got[idx, 4:6])
        print(f"[sum] clustered world, {label} {shape} | rms |acc - f64| / mag: GPU {gpu:.3e} | AVX order {avx:.3e}")
        assert gpu <= avx
