"""The tidal pair-term checker without a GPU: the bound constants are the derived ones, the faithful model of the statement
(tidal_ref.pair_model) stays inside the bound over both case tables of tests/tidal_cases.py with rsq correctly rounded and one
ulp either side, every defective model is rejected by the checker the GPU tests call (tests/test_gpu_tidal_pairs.py) -- on the
range table and again on the slot worlds --, the checker insists on exact zeros and signs, the domain keeps the stated number
of cases and leaves no cell empty, and the float64 reference agrees with exact rational arithmetic."""
import os
from decimal import Decimal

import numpy as np
import pytest

import nbody_amd as nb
import pair_cases as pc
import tidal_cases as tc
import tidal_ref as tr

F32 = np.float32


def world_args(kind, gi, table="probes"):
    sx, sy, _, gm = tc.source(kind, gi)
    if table == "probes":
        pts, rad = tc.points(kind), tc.RADIUS
    else:
        pts = tc.map_expected(kind, gi)["points"]
        rad = tc.map_radius()
    return sx, sy, gm, pts[:, 0], pts[:, 1], rad


def expected(kind, gi, table):
    return tc.expected(kind, gi) if table == "probes" else tc.map_expected(kind, gi)


def rejected(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


def test_the_bound_is_the_derived_one():
    """d: u cubed and three products.  a, b, c: u to the fifth, the five products up to w5 (u * u enters w and w5: counted twice),
    tx or ty, two rounded differences, the fmac onto +0.  One final rounding; the slack is the second-order term."""
    rel_s = pc.REL_S
    assert rel_s == 4 and pc.RSQ_ULPS == 1
    assert tc.D_U == 3 * rel_s + 3 == 15
    assert tc.A_U == tc.B_U == tc.C_U == 5 * rel_s + (1 + 2 + 1 + 1) + 1 + 2 + 1 == 29
    assert tc.FINAL_U == 1
    second_order = 29 ** 2 * pc.U + 4.4 * 4 ** 2 * pc.U + 29 * pc.U + 2.0 ** -25
    assert second_order < 2.0 ** -14 < tc.SECOND_ORDER_U == 2.0 ** -12
    # the bound of one made-up pair, by hand
    parts = tuple(np.array([v]) for v in (2.0, -0.5, 0.125, 5.0))
    e = 29 + 2.0 ** -12, 15 + 2.0 ** -12
    want = np.array([[3 * e[0] * 2 + e[1] * 5 + 1, 3 * e[0] * 0.5 + 1.5, 3 * e[0] * 0.125 + e[1] * 5 + 4.625]]) * pc.U
    assert np.array_equal(tc.bounds(parts), want) and np.array_equal(tc.tensor(parts), [[1.0, -1.5, -4.625]])
    assert pc.NB_G == nb.NB_G


@pytest.mark.parametrize("table", ["probes", "maps"])
@pytest.mark.parametrize("ulps", [-1, 0, 1])
def test_the_faithful_model_stays_inside_the_bound(ulps, table):
    worst_u = worst = 0.0
    for kind, gi in tc.WORLDS:
        e = expected(kind, gi, table)
        got = tr.pair_model(*world_args(kind, gi, table), rsq_ulps=ulps)
        u, r = tc.check(f"model rsq {ulps:+d} ulp {kind} gm {gi}", got, e["parts"], e["mask"], quiet=True)
        worst_u, worst = max(worst_u, u), max(worst, r)
    print(f"[tidal pair] numpy model on the {table} table, rsq {ulps:+d} ulp | worst {worst_u:.2f} u of the parts | worst error / bound {worst:.3f}")
    assert worst > 0.25          # the model does not sit so far inside that the bound says nothing


# "merged diagonal" moves a diagonal component by two roundings (3 * tx, and the difference) of 31: no derived bound can see that, and
# none is asked to.  Its checker is the exact world (test_the_merged_diagonal_is_rejected_on_the_exact_worlds below, and
# tests/test_gpu_tidal_sums.py on the device), where the documented statement has no rounding at all.
BOUND_DEFECTS = tuple(d for d in tr.PAIR_DEFECTS if d != "merged diagonal")


@pytest.mark.parametrize("table", ["probes", "maps"])
@pytest.mark.parametrize("defect", BOUND_DEFECTS)
def test_every_defective_model_is_rejected_on_the_range_tables(defect, table):
    """... in every world of the table, at rsq -1, 0 and +1 ulp: whichever world a route runs, the defect shows."""
    for kind, gi in tc.WORLDS:
        e, args = expected(kind, gi, table), world_args(kind, gi, table)
        for ulps in (-1, 0, 1):
            got = tr.pair_model(*args, rsq_ulps=ulps, defect=defect)
            assert rejected(tc.check, f"{defect} {kind} {gi}", got, e["parts"], e["mask"], quiet=True), (defect, kind, gi, ulps)


def test_the_merged_diagonal_is_rejected_on_the_exact_worlds():
    """one source on tidal_ref.exact_world: the documented statement gives the exactly known tensor, 0 ulp; 3 * tx rounded in
    fp32 misses it on every one of these masses"""
    from test_tidal_cpu import EXACT_MASSES
    p = tr.exact_probe()[0]
    for masses in EXACT_MASSES:
        w = tr.exact_world(masses[:1])
        args = (w[0, 0], w[0, 1], F32(nb.NB_G) * w[0, 6], p[0], p[1], tr.EXACT_SOFT)
        exact = tr.exact_tensor(masses[:1])
        assert max(tr.ulps_off(g, e) for g, e in zip(tr.pair_model(*args)[0], exact)) == 0.0
        assert max(tr.ulps_off(g, e) for g, e in zip(tr.pair_model(*args, defect="merged diagonal")[0], exact)) >= 1.0, masses


@pytest.mark.parametrize("defect", BOUND_DEFECTS)
def test_every_defect_is_rejected_on_the_slot_worlds(defect):
    """the slot worlds' base, the M = 1 world, is held to the same checker: at the 200 probes and at the 200 pixel centres"""
    for pts in (tc.SLOT_POINTS, tr.pixel_points(tc.slot_view())):
        args = tc.slot_args(pts)
        assert tc.in_domain(*args).all()
        parts = tc.reference(*args)
        tc.check("faithful", tr.pair_model(*args), parts, quiet=True)
        assert rejected(tc.check, defect, tr.pair_model(*args, defect=defect), parts, quiet=True), defect


def test_the_checker_insists_on_exact_zeros_signs_and_classes():
    # rows: a general pair; dy = 0 (b = c = 0: xy an exact +0, yy = -d); a cancelling xx (3 a = d up to a remainder of 2^-30 d)
    parts = tuple(np.array(v) for v in ([2.0, 3.0, (1 + 2.0 ** -30) / 3], [0.5, 0.0, 0.25], [0.125, 0.0, 0.5], [5.0, 4.0, 1.0]))
    want = tc.tensor(parts)
    good = want.astype(F32)
    tc.check("good", good, parts, quiet=True)
    bound = tc.bounds(parts)
    for i, v in (((1, 1), 1e-30), ((1, 1), -0.0), ((1, 1), -1e-45), ((0, 0), -1.0), ((0, 2), 4.625), ((0, 1), np.inf), ((2, 2), np.nan),
                 ((0, 0), want[0, 0] + 1.01 * bound[0, 0]), ((1, 2), want[1, 2] * (1 + 19 * pc.U)), ((0, 1), want[0, 1] * (1 + 33 * pc.U))):
        bad = good.copy()
        bad[i] = v
        assert rejected(tc.check, "bad", bad, parts, quiet=True), (i, v)
    ok = good.copy()
    ok[1, 2] = F32(want[1, 2] * (1 + 15 * pc.U))          # yy = -d alone: D_U and the final rounding
    ok[0, 1] = F32(want[0, 1] * (1 + 29 * pc.U))
    # where xx cancels the bound is in the parts: a remainder of either sign and of the parts' rounding size passes ...
    ok[2, 0] = F32(-20 * pc.U)
    tc.check("inside", ok, parts, quiet=True)
    assert abs(want[2, 0]) < bound[2, 0] < 45 * pc.U
    ok[2, 0] = F32(50 * pc.U)                               # ... and one of 50 u of the parts does not
    assert rejected(tc.check, "cancelling xx", ok, parts, quiet=True)
    assert rejected(tc.check, "float64 is no kernel result", want, parts, quiet=True)
    assert rejected(tc.check, "no case", good, parts, np.zeros(3, dtype=bool), quiet=True)


# ---- the domain ------------------------------------------------------------------------------------------------------------------------

def test_the_domain_keeps_the_stated_cases_and_leaves_no_cell_empty():
    assert tc.EXPONENTS == tuple(range(-24, 25, 4)) and tc.TABLE_ROWS == 13 * 5 * 4 * 6 and tc.ROWS == tc.TABLE_ROWS + 13 * 6 == 1638
    assert np.all(tc.RADIUS > 0) and tc.SOFT_MIN == F32(2.0 ** -102) and int((tc.RADIUS == tc.SOFT_MIN).sum()) == tc.TABLE_ROWS // 6
    # "softening negligible": q is the squared distance as rounded
    neg = tc.RADIUS == tc.SOFT_MIN
    d2 = pc.fma32(tc.OFFSET[neg, 1], tc.OFFSET[neg, 1], pc.fma32(tc.OFFSET[neg, 0], tc.OFFSET[neg, 0], 0.0))
    assert np.array_equal(pc.fma32(tc.OFFSET[neg, 1], tc.OFFSET[neg, 1], pc.fma32(tc.OFFSET[neg, 0], tc.OFFSET[neg, 0], tc.SOFT_MIN)), d2)
    shape = (len(tc.EXPONENTS), len(pc.DIRECTIONS), len(pc.RATIOS))
    cells = {kind: np.zeros(shape, dtype=int) for kind in pc.SOURCES}
    total = cancel = alone = 0
    for kind, gi in tc.WORLDS:
        mask = tc.expected(kind, gi)["mask"]
        total += int(mask.sum())
        cancel += int((mask & tc.CANCEL).sum())
        alone += int((mask & tc.D_ALONE).sum())
        np.add.at(cells[kind], tuple(tc.CELL[mask[:tc.TABLE_ROWS]].T), 1)
    assert total == tc.DOMAIN_COUNT == 21082
    assert cancel == 1064 and alone == 4020
    assert np.all(cells["near"].sum(axis=0) > 0) and np.all(cells["near"].sum(axis=(1, 2)) > 0), "a (direction, ratio) cell or an exponent is empty"
    reachable = np.asarray(tc.EXPONENTS) >= -8          # beside a source near 3e4 an offset under its ulp is no offset
    assert np.all(cells["far"][reachable].sum(axis=0) > 0) and np.all(cells["far"][~reachable] == 0)
    # the map table: every view keeps cases, on the axes (an exact zero dx or dy), the diagonals and between them
    total = 0
    seen = np.zeros((len(tc.MAP_VIEWS), 3), dtype=int)
    for kind, gi in tc.WORLDS:
        e = tc.map_expected(kind, gi)
        total += int(e["mask"].sum())
        a, b, c, _ = e["parts"]
        for vi in range(len(tc.MAP_VIEWS)):
            rows = slice(tc.map_rows(vi, 0).start, tc.map_rows(vi, tc.MAP_SOFTS - 1).stop)
            m = e["mask"][rows]
            seen[vi] += int((m & (b[rows] == 0)).sum()), int((m & (a[rows] == c[rows])).sum()), int((m & (b[rows] != 0) & (a[rows] != c[rows])).sum())
    assert total == tc.MAP_DOMAIN_COUNT == 123622 and tc.MAP_ROWS == 26 * 6 * 64
    # the intended centres are the host's: the float32 pixel centres of the view, bit for bit; beside the near source under a
    # power-of-two zoom they are k 2^e exactly
    for kind in pc.SOURCES:
        for vi, (e, z) in enumerate(tc.MAP_VIEWS):
            pts = tc.map_points(kind, vi)
            assert tr.pixel_points(tc.map_view(kind, vi)).tobytes() == pts.tobytes(), (kind, vi)
            if kind == "near" and z == 1.0:
                assert np.array_equal(pts[:tc.MAP_SIDE, 0], (np.arange(tc.MAP_SIDE) - 3.0) * 2.0 ** e)
    assert np.all(seen > 0), seen


def test_the_cancelling_rows_cancel_and_the_d_alone_rows_isolate_d():
    sx, sy, gm, px, py, rad = world_args("near", 4)
    a, b, c, d = tc.expected("near", 4)["parts"]
    dx, dy = px.astype(np.float64), py.astype(np.float64)
    rows = tc.CANCEL
    assert np.all(2 * dx[rows] ** 2 - dy[rows] ** 2 == rad[rows].astype(np.float64))          # s = 2 dx^2 - dy^2, exactly
    assert np.all(np.abs(3 * a[rows] - d[rows]) <= 8 * 2.0 ** -53 * d[rows])                  # xx64 is float64 rounding noise
    assert np.all(tc.bounds((a, b, c, d))[rows, 0] > 40 * pc.U * d[rows])                      # ... and the bound is in the parts
    rows = tc.D_ALONE
    assert np.all(c[rows] == 0) and np.all(b[rows] == 0) and np.array_equal(tc.tensor((a, b, c, d))[rows, 2], -d[rows])


def test_the_domain_ends_where_an_intermediate_leaves_the_normal_range():
    one = F32(1.0)
    assert tc.in_domain(0, 0, one, one, 0, one)[0]
    assert not tc.in_domain(0, 0, one, one, 0, 0)[0]                                 # a softening of 0 cannot be asked
    assert not tc.in_domain(0, 0, one, 0, 0, one)[0]                                 # on the source: pair_cases' "no pair"
    # g u^3 = 2^-75 is normal, g u^5 = 2^-125 is, tx = 2^-100 ... until u^5 takes w5 under 2^-126
    assert tc.in_domain(0, 0, one, F32(2.0 ** 25), 0, one)[0] and not tc.in_domain(0, 0, one, F32(2.0 ** 25.5), 0, one)[0]
    assert pc.in_domain(0, 0, one, F32(2.0 ** 25.5), 0, one)[0]                      # the force statement is still inside there
    assert not tc.in_domain(0, 0, F32(2.0 ** 100), F32(2.0 ** -6), 0, F32(2.0 ** -40))[0]     # w5 = 2^130 overflows; w = 2^118 does not
    assert pc.in_domain(0, 0, F32(2.0 ** 100), F32(2.0 ** -6), 0, F32(2.0 ** -40))[0]
    assert not tc.in_domain(0, 0, F32(2.0 ** -30), F32(2.0 ** 24), 0, one)[0]        # d = 2^-102: under the floor of the parts
    # a padding source adds +0 to all four sums, for any mass: q overflows, rsq(+inf) = +0, and dx * 0 is +0 for dx > 0
    for kind in pc.SOURCES:
        pts = tc.points(kind)
        _, p = tr.pair_model(pc.PAD_AT, pc.PAD_AT, F32(pc.PAD_MASS * pc.NB_G), pts[:, 0], pts[:, 1], tc.RADIUS, parts=True)
        for k in "ABCD":
            assert not p[k].view(np.uint32).any(), k
    # ... and a live term onto +0 keeps its bits through the additions of +0 that follow: 0 + t = t, and +0 + -0 = +0
    assert not pc.fma32(F32(-3.0), F32(0.0), F32(0.0)).view(np.uint32).any()


def test_the_slot_probes_are_in_the_domain_and_the_worlds_hold_one_live_source():
    for pts in (tc.SLOT_POINTS, tr.pixel_points(tc.slot_view())):
        assert pts.shape == (200, 2) and len(np.unique(pts, axis=0)) == 200 and tc.in_domain(*tc.slot_args(pts)).all()
    for m, js in tc.SLOT_COUNTS.items():
        assert max(js) < m
        w = tc.slot_world(m, js[-1])
        assert w.shape == (m, 8) and np.all(w[:, 6] > 0) and int((w[:, 0] != F32(pc.PAD_AT)).sum()) == 1
    assert set(tc.SLOT_COUNTS[2049]) >= {255, 256, 2047, 2048}


# ---- the reference -----------------------------------------------------------------------------------------------------------------------

def test_the_float64_reference_against_exact_rational_arithmetic():
    """on a sample of every world each float64 part is within 12 * 2^-53 of the part formed from exact rational dx, dy, q and a
    60-digit square root"""
    rng = np.random.default_rng(6)
    worst = 0.0
    for kind, gi in tc.WORLDS:
        e, args = tc.expected(kind, gi), world_args(kind, gi)
        for i in rng.choice(np.flatnonzero(e["mask"]), 8, replace=False):
            exact = tc.reference_exact(args[0], args[1], args[2], args[3][i], args[4][i], args[5][i])
            for got, want in zip(e["parts"][:, i], exact):
                if want == 0:
                    assert got == 0
                    continue
                worst = max(worst, abs(float((Decimal(float(got)) - want) / want)))
    print(f"[tidal pair] float64 parts against exact arithmetic | worst {worst / 2.0 ** -53:.2f} x 2^-53")
    assert worst <= 12 * 2.0 ** -53


def test_the_pair_model_is_the_world_model_on_a_one_source_world():
    """tidal_ref.device_model (whole worlds) and pair_model (one pair) share the statement: the same bits on a world of one live
    source among padding, wherever the source sits"""
    pts = tc.SLOT_POINTS
    want = tr.pair_model(*tc.slot_args(pts))
    for m, j in ((1, 0), (19, 7), (300, 256)):
        assert tr.device_model(tc.slot_world(m, j), m, pts, tc.SLOT_SOFT).tobytes() == want.tobytes(), (m, j)
    for variant in tr.VARIANTS[:1]:          # "merged diagonal" is both a world variant and a pair defect
        assert tr.device_model(tc.slot_world(1, 0), 1, pts, tc.SLOT_SOFT, 0, variant).tobytes() == tr.pair_model(*tc.slot_args(pts), defect=variant).tobytes()


# ---- the documents -------------------------------------------------------------------------------------------------------------------------

def test_the_tidal_pair_budget_is_committed_and_cited():
    """DESIGN.md section 5 derives the tidal pair term's bound, lists the sampler's T in the summation scheme and cites one run's
    table; the files it promises exist, and the indexes name them"""
    root = nb.ROOT
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "**The tidal pair term**" in design and "29u" in design and "15u" in design and "E = 1 ulp" in design
    for name in ("profiles/r27_tidal_pair_budget.txt", "tests/tidal_cases.py", "tests/test_tidal_pair_cpu.py", "tests/test_gpu_tidal_pairs.py",
                 "tests/test_gpu_tidal_sums.py"):
        assert os.path.exists(os.path.join(root, name)) and name in design, name
    assert "r27_tidal_pair_budget.txt" in open(os.path.join(root, "profiles", "README.md")).read()
    assert "test_gpu_tidal_pairs.py" in open(os.path.join(root, "README.md")).read()
    assert "profiles/r27_tidal_pair_budget.txt" in open(os.path.join(root, "STATUS.md")).read()
