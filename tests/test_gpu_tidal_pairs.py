"""The pair term of the tidal tensor against float64, to its derived budget, on all six kernels of nbody_amd/csrc/tidal.hip
(needs an MI355X: `pytest -m gpu`; cases, domain, bound and checker: tests/tidal_cases.py; the model, the defective ones and the
checker's teeth without a GPU: tests/tidal_ref.py, tests/test_tidal_pair_cpu.py; the derivation: DESIGN.md section 5 "The tidal
pair term").

A world holds one live source among padding sources whose terms are exact zeros (pair_cases.padded_sources; for the Tidal
statement a source at 2^80 adds +0 to all four sums: test_tidal_pair_cpu.py), so T at a probe is the pair's own term.
Asserted per component: |T - T64| <= (3 * 29 |a| + 15 |d| + |T64|) u for a diagonal one, (3 * 29 |b| + |T64|) u for xy, each
budget + 2^-12 u, with a, b, c, d the float64 parts -- tight where 3 a is close to d --; xy the bits of +0 where dx or dy is an
exact zero; the reference's sign wherever it exceeds the bound.

Routes: tidal_at under tidal_shape SPLIT and WAVE; tidal_map under both (the case table of a map is its own pixel centres,
tidal_cases.map_points: asserted to be tidal_ref.pixel_points' bits before use); SimBatch.tidal_at and .tidal_map of a uniform
and of a ragged ensemble whose live worlds sit between ordinary members of other source counts and sizes.

  (a) range    both tables through every route, every case in the domain, none skipped;
  (b) slots    the live source at index j of M sources, M in 19, 300, 2 049: bit for bit the M = 1 world's term -- the 8-wide
               loop, its tail, the block and the slice ends, independently of the other kernel shape;
  (c) padding  worlds of padding only give three +0;
  and, outside the domain, a probe on a source as g u^5 and then g u^3 overflow: a result is the float64 term within the
  bound or it is not finite, never a finite wrong number.

Every test prints its worst error (`pytest -rP`); profiles/r27_tidal_pair_budget.txt is one run's record.  The assertion is the
derived bound, never a number from that file."""
import numpy as np
import pytest

import nbody_amd as nb
import pair_cases as pc
import tidal_cases as tc
import tidal_ref as tr

pytestmark = pytest.mark.gpu

F32 = np.float32
M = tc.M
SPLIT, WAVE = 1, 2          # the "tidal_shape" hook
SHAPES = {"split": SPLIT, "wave": WAVE}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


class Tally:
    """worst errors and the number of cases a route has been checked on"""

    def __init__(self, label):
        self.label, self.worst_u, self.worst, self.cases = label, 0.0, 0.0, 0

    def add(self, what, got, e):
        assert not np.isnan(got[e["mask"]]).any(), f"{self.label} {what}: a case in the domain was not run (or the device gave NaN there)"
        u, r = tc.check(f"{self.label} {what}", got, e["parts"], e["mask"], quiet=True)
        self.worst_u, self.worst, self.cases = max(self.worst_u, u), max(self.worst, r), self.cases + int(e["mask"].sum())

    def done(self, cases):
        assert self.cases == cases, (self.label, self.cases, cases)
        print(f"[tidal pair] {self.label} | {self.cases} cases | worst {self.worst_u:.2f} u of the parts | worst error / bound "
              f"{self.worst:.3f} | budgets {tc.A_U} u (a, b, c), {tc.D_U} u (d), + {tc.FINAL_U} u final")


def softenings(masks, radius):
    """the distinct softenings of the rows any of the masks keeps: one call each"""
    keep = np.zeros(radius.shape, dtype=bool)
    for m in masks:
        keep |= m
    return np.unique(radius[keep])


def checked_view(kind, vi):
    view = tc.map_view(kind, vi)
    assert tr.pixel_points(view).tobytes() == tc.map_points(kind, vi).tobytes(), (kind, vi)
    return view


# ---- (a) range ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_range_on_tidal_at(shape):
    """One call per softening of the table with ALL the points, so that every case keeps a lane and a tile of its own; the rows
    of that softening are checked."""
    tally = Tally(f"range | tidal_at {shape}")
    sim = nb.SimPipeline(M, M)
    sim.configure(tidal_shape=SHAPES[shape])
    calls = 0
    for kind, gi in tc.WORLDS:
        e, pts = tc.expected(kind, gi), tc.points(kind)
        sim.set_data(tc.world(kind, gi))
        got = np.full((tc.ROWS, 3), np.nan, dtype=F32)
        for soft in softenings([e["mask"]], tc.RADIUS):
            rows = tc.RADIUS == soft
            got[rows] = sim.tidal_at(pts, float(soft))[rows]
            calls += 1
        tally.add(f"{kind} gm {gi}", got, e)
    sim.close()
    tally.done(tc.DOMAIN_COUNT)
    print(f"[tidal pair] range | tidal_at {shape} | {calls} calls")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_range_on_tidal_map(shape):
    tally = Tally(f"range | tidal_map {shape}")
    sim = nb.SimPipeline(M, M)
    sim.configure(tidal_shape=SHAPES[shape])
    views = {kind: [checked_view(kind, vi) for vi in range(len(tc.MAP_VIEWS))] for kind in pc.SOURCES}
    calls = 0
    for kind, gi in tc.WORLDS:
        e = tc.map_expected(kind, gi)
        sim.set_data(tc.world(kind, gi))
        got = np.full((tc.MAP_ROWS, 3), np.nan, dtype=F32)
        for vi, view in enumerate(views[kind]):
            for si, soft in enumerate(tc.map_softenings(vi)):
                rows = tc.map_rows(vi, si)
                if e["mask"][rows].any():
                    got[rows] = sim.tidal_map(view, float(soft)).reshape(-1, 3)
                    calls += 1
        tally.add(f"{kind} gm {gi}", got, e)
    sim.close()
    tally.done(tc.MAP_DOMAIN_COUNT)
    print(f"[tidal pair] range | tidal_map {shape} | {calls} calls")


def ensemble(ragged, live):
    """(SimBatch, indices of the live worlds): the live worlds between ordinary members -- of other source counts in a
    uniform ensemble, of other sizes too in a ragged one (a chain-sized one, N <= 511, and a lane-split-sized one)"""
    n = live[0].shape[0]
    if ragged:
        members = [tc.neighbour(40, 40, 0)] + live[:len(live) // 2] + [tc.neighbour(333, 300, 1)] + live[len(live) // 2:] + [tc.neighbour(700, 600, 2)]
        b = nb.SimBatch.ragged([w.shape[0] for w in members], [int((w[:, 6] > 0).sum()) for w in members])
        b.set_data(members)
    else:
        members = [tc.neighbour(n, n // 2, 0)] + live[:len(live) // 2] + [tc.neighbour(n, n, 1)] + live[len(live) // 2:] + [tc.neighbour(n, 7, 2)]
        b = nb.SimBatch(n, [int((w[:, 6] > 0).sum()) for w in members])
        b.set_data(np.stack(members))
    at = [i for i, w in enumerate(members) if any(w is v for v in live)]
    assert len(at) == len(live) and len(members) == len(live) + 3
    return b, at


def per_member(count, at, values, filler):
    """a list of `count` entries: values[k] for member at[k], `filler` for the ordinary members"""
    out = [filler] * count
    for k, i in enumerate(at):
        out[i] = values[k]
    return out


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_range_on_the_ensembles(ragged):
    """all 18 worlds are members of one ensemble: one launch per softening answers every one of them at its own points, or
    under its own view"""
    name = "ragged" if ragged else "uniform"
    b, at = ensemble(ragged, [tc.world(kind, gi) for kind, gi in tc.WORLDS])
    # probes
    tally = Tally(f"range | SimBatch.tidal_at {name}")
    es = [tc.expected(kind, gi) for kind, gi in tc.WORLDS]
    pts = np.stack(per_member(b.count, at, [tc.points(kind) for kind, _ in tc.WORLDS], tc.points("near")))
    got = np.full((len(es), tc.ROWS, 3), np.nan, dtype=F32)
    for soft in softenings([e["mask"] for e in es], tc.RADIUS):
        rows = tc.RADIUS == soft
        got[:, rows] = b.tidal_at(pts, float(soft))[at][:, rows]
    for (kind, gi), g, e in zip(tc.WORLDS, got, es):
        tally.add(f"{kind} gm {gi}", g, e)
    tally.done(tc.DOMAIN_COUNT)
    # maps
    tally = Tally(f"range | SimBatch.tidal_map {name}")
    es = [tc.map_expected(kind, gi) for kind, gi in tc.WORLDS]
    got = np.full((len(es), tc.MAP_ROWS, 3), np.nan, dtype=F32)
    for vi in range(len(tc.MAP_VIEWS)):
        views = per_member(b.count, at, [checked_view(kind, vi) for kind, _ in tc.WORLDS], tc.map_view("near", vi))
        for si, soft in enumerate(tc.map_softenings(vi)):
            rows = tc.map_rows(vi, si)
            if any(e["mask"][rows].any() for e in es):
                got[:, rows] = b.tidal_map(views, float(soft))[at].reshape(len(es), -1, 3)
    for (kind, gi), g, e in zip(tc.WORLDS, got, es):
        tally.add(f"{kind} gm {gi}", g, e)
    tally.done(tc.MAP_DOMAIN_COUNT)
    b.close()


# ---- (b) slots -----------------------------------------------------------------------------------------------------------------------------

_BASE = {}


def base():
    """(T at the 200 slot probes, T at the 200 centres of the slot view) of the M = 1 world on the split shape, each checked
    against float64 once"""
    if not _BASE:
        sim = nb.SimPipeline(1, 1)
        sim.configure(tidal_shape=SPLIT)
        sim.set_data(tc.slot_world(1, 0))
        view = tc.slot_view()
        at, img = sim.tidal_at(tc.SLOT_POINTS, tc.SLOT_SOFT), sim.tidal_map(view, tc.SLOT_SOFT).reshape(-1, 3)
        sim.close()
        for what, got, pts in (("probes", at, tc.SLOT_POINTS), ("centres", img, tr.pixel_points(view))):
            args = tc.slot_args(pts)
            assert tc.in_domain(*args).all()
            tc.check(f"slots | the M = 1 world, 200 {what}", got, tc.reference(*args))
            got.setflags(write=False)
        _BASE["at"], _BASE["map"] = at, img
    return _BASE["at"], _BASE["map"]


def same_bits(label, got, want):
    got = np.ascontiguousarray(got).reshape(want.shape)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), \
        f"{label}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {got.size} values differ from the M = 1 world's"


@pytest.mark.parametrize("m", [1] + list(tc.SLOT_COUNTS))
def test_slots_on_the_four_pipeline_kernels(m):
    want_at, want_map = base()
    view = tc.slot_view()
    sim = nb.SimPipeline(m, m)
    js = (0,) if m == 1 else tc.SLOT_COUNTS[m]
    for j in js:
        sim.set_data(tc.slot_world(m, j))
        for name, shape in SHAPES.items():
            sim.configure(tidal_shape=shape)
            same_bits(f"tidal_at {name} M={m} j={j}", sim.tidal_at(tc.SLOT_POINTS, tc.SLOT_SOFT), want_at)
            same_bits(f"tidal_map {name} M={m} j={j}", sim.tidal_map(view, tc.SLOT_SOFT), want_map)
    sim.close()
    print(f"[tidal pair] slots | tidal_at + tidal_map, both shapes | M = {m}, j in {js} | the bits of the M = 1 world")


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_slots_on_the_ensembles(ragged):
    """uniform: one ensemble per M, a member per slot; ragged: every M and every slot in one ensemble"""
    want_at, want_map = base()
    view = tc.slot_view()
    groups = [[tc.slot_world(m, j) for m, js in tc.SLOT_COUNTS.items() for j in js]] if ragged else \
        [[tc.slot_world(m, j) for j in js] for m, js in tc.SLOT_COUNTS.items()]
    worlds = 0
    for live in groups:
        b, at = ensemble(ragged, live)
        got_at, got_map = b.tidal_at(tc.SLOT_POINTS, tc.SLOT_SOFT), b.tidal_map(view, tc.SLOT_SOFT)
        b.close()
        for k, i in enumerate(at):
            same_bits(f"SimBatch.tidal_at member {i} (M = {live[k].shape[0]})", got_at[i], want_at)
            same_bits(f"SimBatch.tidal_map member {i} (M = {live[k].shape[0]})", got_map[i], want_map)
        worlds += len(at)
    assert worlds == sum(len(js) for js in tc.SLOT_COUNTS.values())
    print(f"[tidal pair] slots | SimBatch.tidal_at + .tidal_map {'ragged' if ragged else 'uniform'} | {worlds} members | the bits of the M = 1 world")


# ---- (c) padding ---------------------------------------------------------------------------------------------------------------------------

PADDING_SOFTS = (float(tc.SOFT_MIN), 2.0 ** -60, 1.0, 2.0 ** 60)


def all_plus_zero(label, got):
    assert not np.ascontiguousarray(got).view(np.uint32).any(), f"{label}: {int(np.ascontiguousarray(got).view(np.uint32).astype(bool).sum())} values are not +0"


def test_padding_sources_add_three_plus_zero_on_every_route():
    views = [tc.slot_view(), checked_view("far", 11)]
    for m in (1, 19, M):
        part = pc.padded_sources(m, {})
        sim = nb.SimPipeline(m, m)
        sim.set_data(part)
        for name, shape in SHAPES.items():
            sim.configure(tidal_shape=shape)
            for soft in PADDING_SOFTS:
                for kind in pc.SOURCES:
                    all_plus_zero(f"tidal_at {name} M={m} {kind} s={soft}", sim.tidal_at(tc.points(kind), soft))
                for view in views:
                    all_plus_zero(f"tidal_map {name} M={m} s={soft}", sim.tidal_map(view, soft))
        sim.close()
    for ragged in (False, True):
        live = [pc.padded_sources(M, {}), pc.padded_sources(M, {})] if not ragged else [pc.padded_sources(m, {}) for m in (1, 19, M)]
        b, at = ensemble(ragged, live)
        for soft in PADDING_SOFTS:
            all_plus_zero(f"SimBatch.tidal_at ragged={ragged} s={soft}", b.tidal_at(tc.points("far"), soft)[at])
            for view in views:
                all_plus_zero(f"SimBatch.tidal_map ragged={ragged} s={soft}", b.tidal_map(view, soft)[at])
        b.close()


# ---- outside the domain ------------------------------------------------------------------------------------------------------------------

OUTSIDE_STEPS = tuple(range(-40, -127, -2))          # the softening 2^k: g u^5 = 10 * 2^(-2.5 k) passes 2^128 at k = -50, g u^3 at k = -84


@pytest.mark.parametrize("shape", list(SHAPES))
def test_on_a_source_a_result_is_within_the_bound_of_float64_or_it_is_not_finite(shape):
    """One source of G*m = 10 at the origin; probes on it and a denormal distance (2^-140) from it along either axis.  While
    every intermediate of the statement is normal (g u^5 < 2^128: s >= 2^-48) the result is the finite diagonal term
    diag(-G*m s^-1.5) within the bound, with xy = +0.  Below that w5 = g u^5 overflows to +inf and tx = 0 * inf is NaN: the
    statement does not return the finite term the float64 host path still has (include/nbody_tidal.h "On a source").  What
    is asserted there: a component is within the bound of the float64 term or it is not finite -- never a finite wrong
    number.  The classes seen at every step are printed."""
    gm = F32(F32(1.0) * F32(nb.NB_G))
    tiny = F32(2.0 ** -140)
    pts = np.array([[0.0, 0.0], [tiny, 0.0], [0.0, -tiny]], dtype=F32)
    sim = nb.SimPipeline(1, 1)
    sim.configure(tidal_shape=SHAPES[shape])
    sim.set_data(pc.padded_sources(1, {0: (0.0, 0.0, 1.0, 1.0)}))
    seen = []
    for k in OUTSIDE_STEPS:
        soft = 2.0 ** k
        got = sim.tidal_at(pts, soft)
        parts = tc.reference(0.0, 0.0, gm, pts[:, 0], pts[:, 1], np.full(3, soft, dtype=F32))
        with np.errstate(all="ignore"):
            want, bound = tc.tensor(parts), tc.bounds(parts)
            close = np.abs(got.astype(np.float64) - want) <= bound
        finite = np.isfinite(got)
        seen.append((k, "".join("f" if f else "n" if np.isnan(g) else "i" for f, g in zip(finite.ravel(), got.ravel()))))
        assert np.all(close | ~finite), (k, got, want)
        normal = all(bool(pc._normal(tr.statement(0.0, 0.0, gm, 0.0, 0.0, soft, ulps)["w5"])) for ulps in (-1, 0, 1))
        if normal:
            assert finite.all() and np.all(close), (k, got, want)
            assert not got[:, 1].view(np.uint32).any() and got[0, 0] == got[0, 2] < 0, (k, got)
    sim.close()
    runs, last = [], None
    for k, cls in seen:
        if cls != last:
            runs.append(f"from s = 2^{k}: {cls[0:3]} {cls[3:6]} {cls[6:9]}")
            last = cls
    print(f"[tidal pair] outside the domain | tidal_at {shape} | on the source, 2^-140 beside it in x, in y; per probe (xx xy yy): "
          f"f finite and within the bound, n NaN, i infinite | " + "; ".join(runs))
