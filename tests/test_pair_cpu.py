"""The pair-term checker without a GPU: the faithful numpy models of the two statements stay inside the bound of DESIGN.md
section 5 "The pair term" over the whole table of tests/pair_cases.py, every defective model is rejected by the checker the GPU
tests call (tests/test_gpu_pairs.py), the domain keeps the stated number of cases and leaves no cell of the table empty, and the
float64 reference agrees with exact rational arithmetic.  The last test shows what the one-step tolerance of
tests/gpu_common.py does with the same defects."""
import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
import pair_cases as pc
from gpu_common import acc_bound, synth

F32 = np.float32


def world_args(kind, gi):
    s, (px, py) = pc.f32(pc.SOURCES[kind]), pc.tracers(kind)
    return s[0], s[1], pc.source_mass(gi)[1], px, py, pc.RADIUS


def test_the_bound_is_the_derived_one():
    """17 u and 5 u from the roundings counted in pair_cases, with rsq at the stated 1 ulp; the slack is the second-order term."""
    assert (pc.FORCE_U, pc.PHI_U, pc.RSQ_ULPS) == (17, 5, 1)
    assert pc.FORCE_BOUND_U == 17 + 2.0 ** -12 and pc.PHI_BOUND_U == 5 + 2.0 ** -12
    second_order = 17 ** 2 * pc.U + 2 * 4 ** 2 * pc.U + 2.0 ** -26
    assert second_order < 2.0 ** -15 < pc.SECOND_ORDER_U
    assert pc.NB_G == nb.NB_G


@pytest.mark.parametrize("ulps", [-1, 0, 1])
def test_the_faithful_models_stay_inside_the_bound(ulps):
    worst_f = worst_p = 0.0
    for kind, gi in pc.WORLDS:
        e, args = pc.expected(kind, gi), world_args(kind, gi)
        ax, ay = pc.force_model(*args, rsq_ulps=ulps)
        worst_f = max(worst_f, pc.check_force(f"model rsq {ulps:+d} ulp {kind} gm {gi}", np.stack([ax, ay], axis=1), e["acc"], e["mask"]))
        worst_p = max(worst_p, pc.check_phi(f"model rsq {ulps:+d} ulp {kind} gm {gi}", pc.phi_model(*args, rsq_ulps=ulps), e["phi"], e["mask"]))
    print(f"[pair] numpy model, rsq {ulps:+d} ulp | worst force {worst_f:.2f} u, Phi {worst_p:.2f} u")
    # the model must not sit so far inside that the bound says nothing: more than a quarter of it is used
    assert worst_f > pc.FORCE_U / 4 and worst_p > pc.PHI_U / 4


def rejected(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("defect", pc.DEFECTS)
def test_every_defective_force_model_is_rejected(defect):
    """... in every world of the table, at rsq -1, 0 and +1 ulp: whichever world a route runs, the defect shows."""
    for kind, gi in pc.WORLDS:
        e, args = pc.expected(kind, gi), world_args(kind, gi)
        for ulps in (-1, 0, 1):
            ax, ay = pc.force_model(*args, rsq_ulps=ulps, defect=defect)
            assert rejected(pc.check_force, f"{defect} {kind} {gi}", np.stack([ax, ay], axis=1), e["acc"], e["mask"]), (defect, kind, gi, ulps)


@pytest.mark.parametrize("defect", pc.PHI_DEFECTS)
def test_every_defective_phi_model_is_rejected(defect):
    for kind, gi in pc.WORLDS:
        e, args = pc.expected(kind, gi), world_args(kind, gi)
        for ulps in (-1, 0, 1):
            assert rejected(pc.check_phi, f"{defect} {kind} {gi}", pc.phi_model(*args, rsq_ulps=ulps, defect=defect), e["phi"], e["mask"]), \
                (defect, kind, gi, ulps)


@pytest.mark.parametrize("defect", pc.DEFECTS)
def test_every_defect_is_rejected_on_the_slot_tracers_and_the_massive_pairs(defect):
    """The slot worlds and the two-particle worlds are checked by the same checker: the defects show there too (the neighbour's
    radius needs neighbours: the slot tracers; a pair world has none, and is left out for those two)."""
    mask, acc, phi = pc.slot_expected()
    args = (F32(pc.SLOT_SOURCE[0]), F32(pc.SLOT_SOURCE[1]), F32(F32(pc.SLOT_MASS) * F32(pc.NB_G)),
            pc.SLOT_PX[:pc.SLOT_TRACERS], pc.SLOT_PY[:pc.SLOT_TRACERS], pc.SLOT_R[:pc.SLOT_TRACERS])
    ax, ay = pc.force_model(*args, defect=defect)
    assert rejected(pc.check_force, defect, np.stack([ax, ay], axis=1), acc, mask)
    if defect in pc.PHI_DEFECTS:
        assert rejected(pc.check_phi, defect, pc.phi_model(*args, defect=defect), phi, mask)
    if "receiver i ^" in defect:
        return
    got, want = [], []
    for c in pc.pair_cases():
        a, b = c["a"], c["b"]
        ax, ay = pc.force_model(b[0], b[1], F32(b[2] * F32(pc.NB_G)), a[0], a[1], a[3], defect=defect)
        got.append([ax[0], ay[0]])
        want.append(c["want_a"][0])
    assert rejected(pc.check_force, defect, np.asarray(got, dtype=F32), np.asarray(want))


def test_the_checker_insists_on_exact_zeros_signs_and_classes():
    want = np.asarray([[1.0, 0.0], [-2.0, 3.0]])
    good = want.astype(F32)
    assert pc.check_force("good", good, want) == 0.0
    for i, v in (((0, 1), 1e-30), ((0, 1), -1e-45), ((1, 0), 2.0), ((1, 1), np.inf), ((0, 0), np.nan),
                 ((0, 0), 1.0 + 18 * 2.0 ** -24)):
        bad = good.copy()
        bad[i] = v
        assert rejected(pc.check_force, "bad", bad, want), (i, v)
    ok = good.copy()
    ok[1, 1] = F32(3.0 * (1 + 16 * 2.0 ** -24))
    pc.check_force("16 u", ok, want)
    assert rejected(pc.check_force, "float64 is no kernel result", want, want)
    assert rejected(pc.check_force, "no case", good, want, np.zeros(2, dtype=bool))


# ---- the domain --------------------------------------------------------------------------------------------------------------------

def test_the_domain_keeps_the_stated_cases_and_leaves_no_cell_empty():
    assert pc.ROWS == 2520 and len(pc.WORLDS) == 18
    shape = (len(pc.EXPONENTS), len(pc.DIRECTIONS), len(pc.RATIOS))
    cells = {kind: np.zeros(shape, dtype=int) for kind in pc.SOURCES}
    total = 0
    for kind, gi in pc.WORLDS:
        mask = pc.expected(kind, gi)["mask"]
        total += int(mask.sum())
        np.add.at(cells[kind], tuple(pc.CELL[mask].T), 1)
    assert total == pc.DOMAIN_COUNT == 32146
    assert np.all(cells["near"] > 0), "a cell of the table has no case left for any G*m"
    # beside a source near 3e4 an offset under its ulp (2^-9) is no offset: those cells hold nothing, every other one does
    reachable = np.asarray(pc.EXPONENTS) >= -8
    assert np.all(cells["far"][reachable] > 0) and np.all(cells["far"][~reachable] == 0)
    # ... and the far source is where the subtraction rounds: some dx there is not the exact difference
    s, (px, py) = pc.f32(pc.SOURCES["far"]), pc.tracers("far")
    exact = s[0].astype(np.float64) - px.astype(np.float64)
    assert np.any(F32(s[0] - px).astype(np.float64) != exact) and np.all(pc.tracers("near")[0] == pc.OFFSET[:, 0])


def test_the_domain_ends_where_an_intermediate_leaves_the_normal_range():
    one = F32(1.0)
    assert pc.in_domain(0, 0, one, one, 0, 0)[0]
    assert not pc.in_domain(0, 0, one, 0, 0, one)[0]                        # no pair
    assert not pc.in_domain(0, 0, one, F32(2.0 ** -70), 0, 0)[0]            # q = 2^-140: denormal
    assert not pc.in_domain(0, 0, one, F32(2.0 ** 50), 0, 0)[0]             # s * s = 2^-100, u = 2^-150: underflow
    assert not pc.in_domain(0, 0, F32(2.0 ** 100), F32(2.0 ** -20), 0, 0)[0]   # gm * s^3 overflows
    assert not pc.in_domain(0, 0, one, F32(2.0 ** 70), 0, 0)[0]             # q overflows: the padding sources' mechanism
    ax, ay = pc.force_model(pc.PAD_AT, pc.PAD_AT, F32(pc.PAD_MASS * pc.NB_G), pc.tracers("far")[0], pc.tracers("far")[1], pc.RADIUS)
    assert np.all(ax == 0) and np.all(ay == 0) and np.all(pc.phi_model(pc.PAD_AT, pc.PAD_AT, 30.0, *pc.tracers("far"), pc.RADIUS) == 0)


def test_the_slot_tracers_and_the_massive_pairs_are_all_in_the_domain():
    mask, acc, phi = pc.slot_expected(pc.SLOT_TRACERS_LONG)
    assert mask.all() and np.all(acc != 0)
    rows = np.stack([pc.SLOT_PX, pc.SLOT_PY], axis=1)
    assert len(np.unique(rows, axis=0)) == pc.SLOT_TRACERS_LONG and len(np.unique(pc.SLOT_R)) == pc.SLOT_TRACERS_LONG
    cases = pc.pair_cases()
    assert len(cases) == 30 and all(c["ok"] for c in cases)
    assert all(c["a"][3] != c["b"][3] and c["a"][2] != c["b"][2] for c in cases)       # a radius or mass of its own each
    for m, js in pc.SLOT_COUNTS.items():
        w = pc.slot_world(m, js[-1])
        assert w.shape == (m + pc.SLOT_TRACERS, 8) and int((w[:, 6] > 0).sum()) == m and np.all(w[:m, 6] > 0)


# ---- the reference -----------------------------------------------------------------------------------------------------------------

def test_the_float64_reference_against_exact_rational_arithmetic():
    """float64 carries 2^-29 of a float32 rounding: on a sample of every world the float64 term is within 8 * 2^-53 of the
    term formed from exact rational dx, dy, q and a 60-digit square root."""
    from decimal import Decimal
    rng = np.random.default_rng(5)
    worst = 0.0
    for kind, gi in pc.WORLDS:
        e, args = pc.expected(kind, gi), world_args(kind, gi)
        for i in rng.choice(np.flatnonzero(e["mask"]), 12, replace=False):
            exact = pc.reference_exact(args[0], args[1], args[2], args[3][i], args[4][i], args[5][i])
            for got, want in zip((e["acc"][i, 0], e["acc"][i, 1], e["phi"][i]), exact):
                if want == 0:
                    assert got == 0
                    continue
                worst = max(worst, abs(float((Decimal(float(got)) - want) / want)))
    print(f"[pair] float64 reference against exact arithmetic | worst {worst / 2.0 ** -53:.2f} x 2^-53")
    assert worst <= 8 * 2.0 ** -53


# ---- the gap ---------------------------------------------------------------------------------------------------------------------

def test_what_the_one_step_tolerance_does_with_the_same_defects():
    """check_one_step's bound, 1e-4 |acc| + 1e-6 sum|contrib| (1 700 u), on synth(1000), with every pair of the world evaluated
    by a defective model and summed in float64.  A rsq 48 u off passes at every receiver.  A wrong softening passes at most
    of them: the neighbour's radius at 97 % and 96 %, the radius squared at 84 %, all but the receivers with a neighbour
    within a few radii; no softening at 53 %, every massless receiver but those (a massive one's own term turns 0 * inf).  So
    one wrong lane, slot or half of a statement, which reaches a fraction of the receivers, passes with that probability.  Only
    the two defects that change the term's magnitude outright are caught everywhere.  The pair checker rejects all seven
    (above)."""
    part, m = synth(1000)
    acc64, mag = ob.acc_f64(part, m)
    bound = acc_bound(acc64, mag)
    gm = F32(nb.NB_G) * part[:m, 6]
    passes = {}
    for defect in (None,) + pc.DEFECTS:
        acc = np.zeros((part.shape[0], 2))
        for j in range(m):
            ax, ay = pc.force_model(part[j, 0], part[j, 1], gm[j], part[:, 0], part[:, 1], part[:, 7], defect=defect)
            acc[:, 0] += ax
            acc[:, 1] += ay
        passes[defect] = float(np.mean(np.all(np.abs(acc - acc64) <= bound, axis=1)))     # a NaN does not pass
    print("[pair] receivers of synth(1000) at which acc_bound accepts: " + ", ".join(f"{k}: {v:.3f}" for k, v in passes.items()))
    assert passes[None] == 1.0 and passes["rsq 2^-20 off"] == 1.0
    for defect in ("softening dropped", "radius squared", "radius of receiver i ^ 1", "radius of receiver i ^ 64"):
        assert 0.5 < passes[defect] < 1.0, (defect, passes[defect])
    assert passes["one factor s short"] == 0.0 and passes["dy used for dx"] < 0.01


def test_the_exact_head_rows_isolate_the_rsq():
    """On those rows the model's Phi error is the rsq's own plus one rounding: at most 1/2 ulp + u with rsq correctly rounded."""
    args, e = world_args("near", 4), pc.expected("near", 4)
    rows = pc.EXACT_HEAD & e["mask"]
    assert rows.sum() >= 100
    dx, dy, q, _ = pc.head(*args[:2], *args[3:])
    exact = dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2 + pc.RADIUS.astype(np.float64)
    assert np.all(q[rows].astype(np.float64) == exact[rows]) and np.all(dx[rows] == -args[3][rows])
    assert pc.errors_u(pc.phi_model(*args)[rows], e["phi"][rows]).max() <= 2.0
