"""The summation witness has teeth (no GPU): tests/sum_witness.py holds numpy float32 models of the documented two-level sum
(plain over blocks of L sources, compensated over the block totals, plain joins of the slices, parts and passes) and of two
defective ones (one plain running sum; the same blocks with plain totals), and the bound E(shape) that
tests/test_gpu_sums.py asserts on the MI355X.  Here the terms are stood in by arbitrary 24-bit float32 values -- 1.0, a mantissa
of all ones and seeded random ones -- and for every case of sum_witness.CASES, which is the table the GPU file runs:

  * the documented model stays inside E, for every position of the big term and every shape;
  * at every case marked `teeth` BOTH defective models leave E (for the field sampler and the diagnostics the defect is float32
    block totals, and the bound is theirs: 1 ulp, or the float64 model's own in-block error plus 2^-52 relative);
  * the exactly-once condition |sum - M t| < t / 4 holds for the documented model at every source count of the GPU suite's sweeps,
    and fails as soon as one term is removed or added twice, at the first, the last and a block-edge index.

The one-workgroup chain and the ensembles have no case with teeth for the compensation: at most 3 000 sources are twelve
blocks of 256, three ulps of small terms in all, cut into 4 to 64 slices, so no slice holds enough blocks for a lost
compensation to show above E.  They run pattern 1, and pattern 2 for the bound alone."""
from fractions import Fraction

import numpy as np
import pytest

import sum_witness as sw
from test_gpu_parity import GRANULE_COUNTS, GRANULE_KNOBS, SWEEP_COUNTS, SWEEP_KNOBS
from test_gpu_field import SOURCES as FIELD_SOURCES

F32 = np.float32


def stand_ins():
    """small terms with 24-bit mantissas: 1.0, all ones, and two seeded ones"""
    rng = np.random.default_rng(20240)
    mant = [1 << 23, (1 << 24) - 1] + [int(v) | (1 << 23) for v in rng.integers(0, 1 << 23, 2)]
    return [F32(np.ldexp(float(m), -50)) for m in mant]


T_SMALL = stand_ins()
FAMILIES = ("classic", "lane", "sharded", "field", "diag")
IDS = [f"{c['family']}-{c['pattern']}-{c['at']}-M{c['m']}-" + "-".join(f"{k}{v}" for k, v in c["shape"].items()) for c in sw.CASES]


def within(c, values, exact, scale):
    if c["family"] == "diag":
        return all(abs(Fraction(float(v)) - exact) <= diag_bound(c, exact, scale) for v in values)
    return all(abs(sw.err_ulps(v, exact, scale)) <= sw.case_E(c) for v in values)


def diag_bound(c, exact, scale):
    # the float64 scheme's own error is what its fp32 blocks lose; the float64 additions of <= 257 values add 2^-52 relative
    x = diag_bound.terms
    return abs(Fraction(float(sw.field_model(x, "f64"))) - exact) + abs(scale) * Fraction(1, 2 ** 52)


def test_every_family_has_a_case_with_teeth():
    for fam in FAMILIES:
        assert any(c["teeth"] for c in sw.CASES if c["family"] == fam), fam
    assert any(c["teeth"] and c["m"] == 65536 for c in sw.CASES if c["family"] == "classic")
    assert any(c["teeth"] and c["shape"] == dict(w=4, lanes=2) for c in sw.CASES)
    assert not any(c["teeth"] for c in sw.CASES if c["shape"].get("w") == 16)     # labelled: bound only
    assert sw.big_shift(256) == 33 and sw.big_shift(128) == 32


@pytest.mark.parametrize("c", sw.CASES, ids=IDS)
def test_the_documented_scheme_stays_inside_E_and_the_defects_do_not(c):
    caught = dict(plain=0, blocks=0)
    for t in T_SMALL:
        x, exact, scale = sw.case_terms(c, t)
        diag_bound.terms = x
        good = sw.case_model(c, x, "kahan")
        assert within(c, good, exact, scale), (c, float(t), [sw.err_ulps(v, exact, scale) for v in good], sw.case_E(c))
        if not c["teeth"]:
            continue
        for scheme in ("plain", "blocks"):
            bad = sw.case_model(c, x, scheme)
            caught[scheme] += not within(c, bad, exact, scale)
    if c["teeth"]:
        # The force kernels' defects lose whole ulps of the big term at every stand-in.  Float32 totals in the sampler and the
        # diagnostics lose the two to five ulps of their slice's other seven blocks and then round eight times, which can land
        # back inside the bound by chance (one stand-in of four does, at 0.31 ulp): a GPU case measures at least four distinct
        # terms (x and y of three tracer positions), so three stand-ins of four is what "caught" means there.
        need = len(T_SMALL) - (1 if c["family"] in ("field", "diag") else 0)
        assert min(caught.values()) >= need, (c, caught)


def test_the_field_potential_bound_is_one_ulp_and_float32_totals_break_it():
    """Phi: the same sampler with a one-component term; 1 ulp of float32 for float64 totals, not for float32 totals."""
    c = sw.case("field", 16384, True, at="first")
    caught = 0
    for t in T_SMALL:
        x, exact, _ = sw.case_terms(c, t)
        assert abs(sw.err_ulps(F32(sw.field_model(x, "f64")), exact)) <= 1.0
        caught += abs(sw.err_ulps(F32(sw.field_model(x, "f32")), exact)) > 1.0
    assert caught >= len(T_SMALL) - 1


# ---- pattern 1: every source exactly once ----------------------------------------------------------------------------------

def shapes_of_pattern_1():
    out = [(m, dict(knobs, unit=64)) for m in SWEEP_COUNTS for knobs in SWEEP_KNOBS]
    out += [(m, dict(knobs, unit=u)) for m in GRANULE_COUNTS for knobs in GRANULE_KNOBS for u in (8, 16, 32, 64)]
    return out


def model_of(knobs, x):
    return sw.classic_model(x, "kahan", w=knobs["w"], split=knobs.get("split", 1), passes=knobs.get("passes", 1), unit=knobs["unit"])


def once(value, m, t):
    return abs(Fraction(float(value)) - m * Fraction(float(t))) < Fraction(float(t)) / 4


def test_the_exactly_once_condition_is_met_by_the_documented_scheme_at_every_count():
    assert max(SWEEP_COUNTS + GRANULE_COUNTS + FIELD_SOURCES + [3000]) <= sw.EXACTLY_ONCE_MAX
    # worst case of the documented scheme over M <= 4 500 equal terms, in units of one term: 0.07 < 1 / 4
    assert sw.exactly_once_bound_in_terms(sw.EXACTLY_ONCE_MAX) < 0.08
    t = T_SMALL[1]                      # the mantissa of all ones rounds at every addition
    for m, knobs in shapes_of_pattern_1():
        assert once(model_of(knobs, np.full(m, t, dtype=F32)), m, t), (m, knobs)
    for m in [c for c in FIELD_SOURCES if c > 0]:
        assert once(sw.field_model(np.full(m, t, dtype=F32)), m, t), m


@pytest.mark.parametrize("m", [257, 1031, 2111])
def test_one_term_removed_or_added_twice_breaks_the_exactly_once_condition(m):
    for t in T_SMALL:
        x = np.full(m, t, dtype=F32)
        for knobs in SWEEP_KNOBS:
            knobs = dict(knobs, unit=64)
            for i in (0, 255, 256, m - 1):          # the first, a block edge on either side, the last
                assert not once(model_of(knobs, np.delete(x, i)), m, t), (m, knobs, i, "removed")
                assert not once(model_of(knobs, np.insert(x, i, t)), m, t), (m, knobs, i, "twice")
        assert not once(sw.field_model(np.delete(x, 0)), m, t) and not once(sw.field_model(np.insert(x, 256, t)), m, t)


def test_the_small_ensemble_sizes_give_the_compensation_no_teeth():
    """3 000 sources in the ensembles' (W, H) = (16, 4): the defective block model stays inside E, which is why those families
    carry the bound only."""
    c = sw.case("lane", 3000, False, at="first", w=16, lanes=4)
    for t in T_SMALL:
        x, exact, scale = sw.case_terms(c, t)
        for scheme in sw.SCHEMES:
            assert abs(sw.err_ulps(sw.lane_split_model(x, scheme, 16, 4), exact, scale)) <= sw.case_E(c)
