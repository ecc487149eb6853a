"""The pair term of the force and potential kernels against float64, to its ulp budget, on every route that holds a copy of a
statement or of the code around it (needs an MI355X: `pytest -m gpu`; cases, domain, bound and models: tests/pair_cases.py; the
checker's teeth without a GPU: tests/test_pair_cpu.py; the derivation: DESIGN.md section 5 "The pair term").

A world holds one live source among padding sources whose terms are exact zeros, and massless tracers: a tracer's acc after
update(1, 0.0) -- positions stay put, acc is stored -- is the pair's term itself, and so are its Phi and the field at its
position.  Asserted: every component within 17 u (Phi: 5 u) of the float64 term, u = 2^-24; an exact zero where the term is
zero; the term's sign.

  (a) range   the table (separations 2^-40 ... 2^40, five directions, six radius ratios, four mantissas, exact and rounding
              subtractions, nine G*m) through every route, every case in the domain, none skipped;
  (b) slots   the live source at index j of M sources in front of 200 tracers with positions and radii of their own: bit for bit
              the term of the M = 1 world -- a pair's bits do not depend on which copy of the statement evaluated it;
  (c) massive receivers: two live particles, each receives the other's term; the pair in one block and in two, which is the
              masked and the unmasked Phi statement.

Every test prints its worst error in u (`pytest -rP`); profiles/r15_pair_budget.txt is one run's record.  The assertion is the
derived bound, never a number from that file."""
import numpy as np
import pytest

import nbody_amd as nb
import pair_cases as pc

pytestmark = pytest.mark.gpu

F32 = np.float32
M, J = pc.RANGE_M, pc.RANGE_J
CHAIN_ROWS = 360          # tracers per world of at most 512 particles: 2 520 = 7 * 360, 130 + 360 = 490
SPLIT, WAVE = 1, 2        # the "field_shape" / "gravity_shape" hooks


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


# ---- the step routes of one pipeline ---------------------------------------------------------------------------------------------

# name -> (knobs, steps per call).  The chain runs calls of two steps or more; with dt = 0 the second step repeats the first.
PIPE_ROUTES = {}
for _k, _w in ((1, 1), (1, 16), (2, 4), (2, 16)):
    for _v in (0, 1):
        PIPE_ROUTES[f"classic-k{_k}w{_w}-variant{_v}"] = (dict(k=_k, w=_w, split=1, variant=_v, lanes=1, fused_chain=0), 1)
PIPE_ROUTES["split3-finish"] = (dict(k=2, w=4, split=3, variant=1, lanes=1, fused_finish=0, fused_chain=0), 1)
PIPE_ROUTES["passes2"] = (dict(k=2, w=4, split=1, passes=2, variant=1, lanes=1, fused_chain=0), 1)
PIPE_ROUTES["lanes2-w4"] = (dict(lanes=2, w=4, fused_chain=0), 1)
PIPE_ROUTES["lanes4-w8"] = (dict(lanes=4, w=8, fused_chain=0), 1)
PIPE_ROUTES["lanes8-w16"] = (dict(lanes=8, w=16, fused_chain=0), 1)
PIPE_ROUTES["chain"] = (dict(fused_chain=1), 2)


class Pipe:
    """one SimPipeline pinned to a route, reused for every world of its size"""

    def __init__(self, n, m, route):
        self.knobs, self.steps = PIPE_ROUTES[route]
        self.n, self.m, self.route = n, m, route
        self.sim = nb.SimPipeline(n, m)
        self.sim.configure(**self.knobs)

    def acc(self, part):
        self.sim.set_data(part)
        self.sim.update(self.steps, 0.0)
        out = self.sim.get_data()
        self.route_taken()
        assert np.array_equal(out[:, 6:8], part[:, 6:8])
        return out[:, 4:6]

    def route_taken(self):
        shape, k = self.sim.launch_shape(), self.knobs
        if k.get("fused_chain") == 1:
            assert self.sim.fused_steps() == self.steps, (self.route, self.sim.fused_steps())
            return
        assert self.sim.fused_steps() == 0
        assert shape["lanes"] == k["lanes"] and shape["w"] == k["w"], (self.route, shape)
        if k["lanes"] == 1:
            assert shape["k"] == k["k"] and shape["variant"] == ("smem" if k["variant"] else "lds"), (self.route, shape)
            assert shape["split"] == k["split"], (self.route, shape)
            assert (self.sim.finish_launches() > 0) == (k["split"] > 1), (self.route, self.sim.finish_launches())
            assert self.sim.last_step_ms()[1] == min(k.get("passes", 1), -(-self.m // 64)), (self.route, self.sim.last_step_ms())

    def close(self):
        self.sim.close()


def slices_for(route):
    """the table in one world, or, for the chain (N <= 512), in seven"""
    return [slice(i, i + CHAIN_ROWS) for i in range(0, pc.ROWS, CHAIN_ROWS)] if route == "chain" else [slice(0, pc.ROWS)]


class Tally:
    """worst errors and the number of cases a test has checked"""

    def __init__(self, label):
        self.label, self.force, self.phi, self.cases_f, self.cases_p = label, 0.0, 0.0, 0, 0

    def add_force(self, what, acc, e, rows=slice(None)):
        mask = e["mask"][rows]
        if mask.any():
            self.force = max(self.force, pc.check_force(f"{self.label} {what}", acc, e["acc"][rows], mask, quiet=True))
            self.cases_f += int(mask.sum())

    def add_phi(self, what, phi, e, rows=slice(None)):
        mask = e["mask"][rows]
        if mask.any():
            self.phi = max(self.phi, pc.check_phi(f"{self.label} {what}", phi, e["phi"][rows], mask, quiet=True))
            self.cases_p += int(mask.sum())

    def done(self, force=True, phi=False, cases=pc.DOMAIN_COUNT):
        line = f"[pair] {self.label}"
        if force:
            assert self.cases_f == cases, (self.label, self.cases_f, cases)
            line += f" | force: {self.cases_f} cases, worst {self.force:.2f} u, bound {pc.FORCE_BOUND_U:g} u"
        if phi:
            assert self.cases_p == cases, (self.label, self.cases_p, cases)
            line += f" | Phi: {self.cases_p} cases, worst {self.phi:.2f} u, bound {pc.PHI_BOUND_U:g} u"
        print(line)


# ---- the padding ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", list(PIPE_ROUTES))
def test_padding_sources_add_exact_zeros_on_every_step_route(route):
    for m in (1, 19, M):
        for kind in pc.SOURCES:
            for rows in slices_for(route)[:2]:
                part = pc.padding_world(m, kind)
                part = np.concatenate([part[:m], part[m:][rows]])
                pipe = Pipe(part.shape[0], m, route)
                acc = pipe.acc(part)
                pipe.close()
                assert np.all(acc == 0), f"{route} M={m} {kind}: {int((acc != 0).sum())} values are not zero"


def test_padding_sources_add_exact_zeros_to_phi_and_the_field():
    for m in (1, 19, M):
        part = pc.padding_world(m)
        n = part.shape[0]
        sim = nb.SimPipeline(n, m)
        sim.set_data(part)
        assert np.all(sim.potential()[m:] == 0)
        for shape in (SPLIT, WAVE):
            sim.configure(field_shape=shape, gravity_shape=shape)
            for soft in (2.0 ** -100, 2.0 ** -60, 1.0, 2.0 ** 60):
                assert np.all(sim.potential_at(part[m:, 0:2], soft) == 0) and np.all(sim.acceleration_at(part[m:, 0:2], soft) == 0)
        sim.close()
        b = nb.SimBatch(m + CHAIN_ROWS, [m, m])
        b.set_data(np.stack([np.concatenate([part[:m], part[m:][rows]]) for rows in slices_for("chain")[:2]]))
        b.update(1, 0.0)
        assert np.all(b.get_data()[:, :, 4:6] == 0) and np.all(b.potential()[:, m:] == 0)
        b.close()


# ---- (a) range ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", list(PIPE_ROUTES))
def test_range_on_every_step_route(route):
    tally = Tally(f"range | {route}")
    for rows in slices_for(route):
        pipe = Pipe(M + rows.stop - rows.start, M, route)
        for kind, gi in pc.WORLDS:
            acc = pipe.acc(pc.range_world(kind, gi, rows=rows))
            tally.add_force(f"{kind} gm {gi} rows {rows.start}", acc[M:], pc.expected(kind, gi), rows)
        pipe.close()
    tally.done()


@pytest.mark.parametrize("overlap", [0, 1], ids=["plain", "overlapped"])
def test_range_on_a_sharded_group_of_two(overlap):
    tally = Tally(f"range | LocalShardGroup P=2 overlap={overlap}")
    group = nb.LocalShardGroup(M + pc.ROWS, M, 2, overlap=overlap)
    for kind, gi in pc.WORLDS:
        group.set_data(pc.range_world(kind, gi))
        group.step(1, 0.0)
        outs = [group.get_data(r) for r in range(2)]
        assert outs[0].tobytes() == outs[1].tobytes(), "the ranks hold different bytes"
        tally.add_force(f"{kind} gm {gi}", outs[0][M:, 4:6], pc.expected(kind, gi))
    group.close()
    tally.done()


def ensemble(members, ragged):
    """members: [(kind, gi, rows)] -> (acc per member, Phi per member, launch shape)"""
    worlds = [pc.range_world(kind, gi, rows=rows) for kind, gi, rows in members]
    if ragged:
        b = nb.SimBatch.ragged([w.shape[0] for w in worlds], [M] * len(worlds))
        b.set_data(worlds)
    else:
        b = nb.SimBatch(worlds[0].shape[0], [M] * len(worlds))
        b.set_data(np.stack(worlds))
    phi = b.potential()
    b.update(1, 0.0)
    got, shape = b.get_data(), b.launch_shape()
    b.close()
    return [got[i][M:, 4:6] for i in range(len(worlds))], [phi[i][M:] for i in range(len(worlds))], shape


def check_ensemble(label, members, ragged, paths):
    tally = Tally(label)
    acc, phi, shape = ensemble(members, ragged)
    seen = {g["path"] for g in shape["groups"]} if ragged else {shape["path"]}
    assert seen == set(paths), shape
    for (kind, gi, rows), a, p in zip(members, acc, phi):
        tally.add_force(f"{kind} gm {gi} rows {rows.start}", a, pc.expected(kind, gi), rows)
        tally.add_phi(f"{kind} gm {gi} rows {rows.start}", p, pc.expected(kind, gi), rows)
    tally.done(phi=True)


def test_range_on_a_uniform_ensemble_of_one_workgroup_worlds():
    """126 members of 490 particles: batch_chain_kernel<BatchParams>, and ensemble_phi_kernel<EnsembleDiagParams> for SimBatch.potential()"""
    check_ensemble("range | SimBatch N=490 (chain path) + SimBatch.potential()",
                   [(kind, gi, rows) for kind, gi in pc.WORLDS for rows in slices_for("chain")], False, ["chain"])


def test_range_on_a_uniform_ensemble_of_lane_split_worlds():
    """18 members of 2 650 particles: batch_lane_split_kernel<16, 4, BatchParams>"""
    check_ensemble("range | SimBatch N=2650 (lanes path) + SimBatch.potential()",
                   [(kind, gi, slice(0, pc.ROWS)) for kind, gi in pc.WORLDS], False, ["lanes"])


def test_range_on_a_ragged_ensemble():
    """per world one member of 490 and two of 1 210 particles: batch_chain_kernel and batch_lane_split_kernel<8, 8> for RaggedParams,
    one launch group each, and ensemble_phi_kernel<RaggedDiagParams>"""
    cuts = (slice(0, 360), slice(360, 1440), slice(1440, pc.ROWS))
    check_ensemble("range | SimBatch.ragged N in (490, 1210, 1210) + potential()",
                   [(kind, gi, rows) for kind, gi in pc.WORLDS for rows in cuts], True, ["chain", "lanes"])


def test_range_on_the_per_particle_potential():
    """potential_kernel: a tracer's Phi_i with its own radius.  On the rows whose dx, dy and q are exact, beside a G*m that is a
    power of two (the product G*m * s is then exact as well), the error is the rsq's own and nothing else: rho, printed, and
    held to the 1 ulp = 2 u the bound is derived from.  If a route left the bound, this says whether v_rsq_f32 did it."""
    tally = Tally("range | potential()")
    sim = nb.SimPipeline(M + pc.ROWS, M)
    rho, rows_seen = 0.0, 0
    for kind, gi in pc.WORLDS:
        sim.set_data(pc.range_world(kind, gi))
        phi = sim.potential()[M:]
        e = pc.expected(kind, gi)
        tally.add_phi(f"{kind} gm {gi}", phi, e)
        if kind == "near" and np.frexp(pc.source_mass(gi)[1])[0] == 0.5:
            rows = pc.EXACT_HEAD & e["mask"]
            rho = max(rho, float(pc.errors_u(phi[rows], e["phi"][rows]).max()))
            rows_seen += int(rows.sum())
    sim.close()
    tally.done(force=False, phi=True)
    print(f"[pair] range | potential() on the {rows_seen} rows with exact dx, dy, q and G*m * s | worst {rho:.2f} u = rho, the error of "
          f"v_rsq_f32 alone | 1 ulp allows {2 * pc.RSQ_ULPS} u")
    assert rows_seen >= 300 and rho <= 2 * pc.RSQ_ULPS


@pytest.mark.parametrize("shape", [SPLIT, WAVE], ids=["split", "wave"])
def test_range_on_the_field_sampler(shape):
    """acceleration_at and potential_at with the tracers as probe points.  The softening is per call: one call per radius of the
    table with ALL the points, so that every case keeps a lane and a tile of its own; the rows of that radius are checked.  The
    samplers take a softening > 0 only (include/nbody_field.h): the rows with radius 0 cannot be asked of them."""
    tally = Tally(f"range | acceleration_at + potential_at shape {shape}")
    reachable = sum(int((pc.expected(kind, gi)["mask"] & (pc.RADIUS > 0)).sum()) for kind, gi in pc.WORLDS)
    sim = nb.SimPipeline(M + pc.ROWS, M)
    sim.configure(field_shape=shape, gravity_shape=shape)
    calls = 0
    for kind, gi in pc.WORLDS:
        part, e = pc.range_world(kind, gi), pc.expected(kind, gi)
        e = dict(e, mask=e["mask"] & (pc.RADIUS > 0))
        sim.set_data(part)
        pts = part[M:, 0:2]
        g, phi = np.full((pc.ROWS, 2), np.nan, dtype=F32), np.full(pc.ROWS, np.nan, dtype=F32)
        for soft in np.unique(pc.RADIUS[e["mask"]]):
            rows = pc.RADIUS == soft
            g[rows] = sim.acceleration_at(pts, float(soft))[rows]
            phi[rows] = sim.potential_at(pts, float(soft))[rows]
            calls += 2
        tally.add_force(f"{kind} gm {gi}", g, e)
        tally.add_phi(f"{kind} gm {gi}", phi, e)
    sim.close()
    tally.done(phi=True, cases=reachable)
    print(f"[pair] range | field sampler shape {shape} | {calls} calls")


def test_a_denormal_q_is_flushed_by_the_rsq():
    """Outside the domain, for the record (include/nbody_hip.h "Non-finite state"): q = 2^-140 beside G*m = 1.  v_rsq_f32 flushes
    a denormal input to zero, so Phi is -inf where float64 gives -2^70; were it kept, Phi would be within the bound of that."""
    part = np.concatenate([pc.padded_sources(1, {0: (0.0, 0.0, 0.1, 1.0)}), pc.tracer_rows([2.0 ** -70], [0.0], [0.0])])
    sim = nb.SimPipeline(2, 1)
    sim.set_data(part)
    phi = sim.potential()[1]
    sim.close()
    kept = abs(float(phi) + 2.0 ** 70) <= pc.PHI_BOUND_U * pc.U * 2.0 ** 70
    print(f"[pair] measured: q = 2^-140 (denormal), G*m = 1 | Phi = {phi!r} | float64 {-2.0 ** 70!r} | "
          f"{'kept' if kept else 'flushed to zero by v_rsq_f32' if phi == -np.inf else 'neither'}")
    assert phi == -np.inf or kept


# ---- (b) slots --------------------------------------------------------------------------------------------------------------------------

_BASE = {}


def base(tracers=pc.SLOT_TRACERS):
    """(acc, Phi) of the slot tracers in the M = 1 world on the plainest route, checked against float64 once"""
    if tracers not in _BASE:
        part = pc.slot_world(1, 0, tracers)
        pipe = Pipe(part.shape[0], 1, "classic-k1w1-variant1")
        acc = pipe.acc(part)[1:].copy()
        phi = pipe.sim.potential()[1:].copy()
        pipe.close()
        mask, want_acc, want_phi = pc.slot_expected(tracers)
        worst = pc.check_force("slots | M = 1", acc, want_acc, mask, quiet=True), pc.check_phi("slots | M = 1", phi, want_phi, mask, quiet=True)
        print(f"[pair] slots | the M = 1 world, {tracers} tracers | force worst {worst[0]:.2f} u | Phi worst {worst[1]:.2f} u")
        for a in (acc, phi):
            a.setflags(write=False)
        _BASE[tracers] = (acc, phi)
    return _BASE[tracers]


def same_bits(label, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), \
        f"{label}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {got.size} values differ from the M = 1 world's"


SLOTS = [(m, j) for m, js in pc.SLOT_COUNTS.items() for j in js]


@pytest.mark.parametrize("route", list(PIPE_ROUTES))
def test_slots_on_every_step_route(route):
    want = base()[0]
    one = Pipe(1 + pc.SLOT_TRACERS, 1, route)
    same_bits(f"{route} M=1", one.acc(pc.slot_world(1, 0))[1:], want)
    one.close()
    for m, js in pc.SLOT_COUNTS.items():
        pipe = Pipe(m + pc.SLOT_TRACERS, m, route)
        for j in js:
            same_bits(f"{route} M={m} j={j}", pipe.acc(pc.slot_world(m, j))[m:], want)
        pipe.close()
    print(f"[pair] slots | {route} | {1 + len(SLOTS)} worlds x {pc.SLOT_TRACERS} tracers | the bits of the M = 1 world")


@pytest.mark.parametrize("overlap", [0, 1], ids=["plain", "overlapped"])
def test_slots_on_a_sharded_group_of_two(overlap):
    want = base()[0]
    for m, js in pc.SLOT_COUNTS.items():
        group = nb.LocalShardGroup(m + pc.SLOT_TRACERS, m, 2, overlap=overlap)
        for j in js:
            group.set_data(pc.slot_world(m, j))
            group.step(1, 0.0)
            same_bits(f"sharded overlap={overlap} M={m} j={j}", group.get_data(1)[m:, 4:6], want)
        group.close()
    print(f"[pair] slots | LocalShardGroup P=2 overlap={overlap} | {len(SLOTS)} worlds | the bits of the M = 1 world")


@pytest.mark.parametrize("tracers,path", [(pc.SLOT_TRACERS, "chain"), (pc.SLOT_TRACERS_LONG, "lanes")])
def test_slots_on_the_ensembles_and_their_potential(tracers, path):
    want_acc, want_phi = base(tracers)
    for m, js in pc.SLOT_COUNTS.items():
        b = nb.SimBatch(m + tracers, [m] * len(js))
        b.set_data(np.stack([pc.slot_world(m, j, tracers) for j in js]))
        phi = b.potential()
        b.update(1, 0.0)
        got, shape = b.get_data(), b.launch_shape()
        b.close()
        assert shape["path"] == path, shape
        for i, j in enumerate(js):
            same_bits(f"SimBatch {path} M={m} j={j}", got[i, m:, 4:6], want_acc)
            same_bits(f"SimBatch.potential() {path} M={m} j={j}", phi[i, m:], want_phi)
    print(f"[pair] slots | SimBatch ({path} path) + SimBatch.potential() | {len(SLOTS)} members x {tracers} tracers | the bits of the M = 1 world")


def test_slots_on_the_potential_and_the_field_sampler():
    """potential(): every tracer with its own radius.  The samplers take one softening per call: the M = 1 world's sampler
    result with the same softening is the base, itself within the bound of float64."""
    want_phi = base()[1]
    soft = 0.75
    args = (F32(pc.SLOT_SOURCE[0]), F32(pc.SLOT_SOURCE[1]), F32(F32(pc.SLOT_MASS) * F32(pc.NB_G)),
            pc.SLOT_PX[:pc.SLOT_TRACERS], pc.SLOT_PY[:pc.SLOT_TRACERS], np.full(pc.SLOT_TRACERS, soft, dtype=F32))
    ax, ay, ph = pc.reference(*args)
    assert pc.in_domain(*args).all()
    pts = np.stack([args[3], args[4]], axis=1)
    field = {}
    for m, js in {1: (0,), **pc.SLOT_COUNTS}.items():
        sim = nb.SimPipeline(m + pc.SLOT_TRACERS, m)
        for j in js:
            sim.set_data(pc.slot_world(m, j))
            same_bits(f"potential() M={m} j={j}", sim.potential()[m:], want_phi)
            for shape in (SPLIT, WAVE):
                sim.configure(field_shape=shape, gravity_shape=shape)
                g, phi = sim.acceleration_at(pts, soft), sim.potential_at(pts, soft)
                if m == 1:
                    field[shape] = (g, phi)
                    worst = pc.check_force("sampler M = 1", g, np.stack([ax, ay], axis=1), quiet=True), pc.check_phi("sampler M = 1", phi, ph, quiet=True)
                    print(f"[pair] slots | field sampler shape {shape}, M = 1 | force worst {worst[0]:.2f} u | Phi worst {worst[1]:.2f} u")
                same_bits(f"acceleration_at shape {shape} M={m} j={j}", g, field[shape][0])
                same_bits(f"potential_at shape {shape} M={m} j={j}", phi, field[shape][1])
        sim.close()
    same_bits("the two sampler shapes", field[SPLIT][0], field[WAVE][0])
    same_bits("the two sampler shapes", field[SPLIT][1], field[WAVE][1])
    print(f"[pair] slots | potential() + acceleration_at + potential_at, both shapes | {1 + len(SLOTS)} worlds | the bits of the M = 1 world")


# ---- (c) massive receivers ----------------------------------------------------------------------------------------------------------------

PAIRS = pc.pair_cases()
WANT_ACC = {w: np.stack([c[w][0] for c in PAIRS]) for w in ("want_a", "want_b")}
WANT_PHI = {w: np.asarray([c[w][1] for c in PAIRS]) for w in ("want_a", "want_b")}


def check_pairs(label, acc_a, acc_b, phi_a=None, phi_b=None):
    f = max(pc.check_force(f"{label} A", np.stack(acc_a), WANT_ACC["want_a"], quiet=True),
            pc.check_force(f"{label} B", np.stack(acc_b), WANT_ACC["want_b"], quiet=True))
    line = f"[pair] massive receivers | {label} | {2 * len(PAIRS)} receivers | force worst {f:.2f} u"
    if phi_a is not None:
        p = max(pc.check_phi(f"{label} A", np.asarray(phi_a, dtype=F32), WANT_PHI["want_a"], quiet=True),
                pc.check_phi(f"{label} B", np.asarray(phi_b, dtype=F32), WANT_PHI["want_b"], quiet=True))
        line += f" | Phi worst {p:.2f} u"
    print(line)


@pytest.mark.parametrize("place", list(pc.PAIR_PLACES))
@pytest.mark.parametrize("route", list(PIPE_ROUTES))
def test_massive_receivers_on_every_step_route(route, place):
    assert all(c["ok"] for c in PAIRS)
    ia, ib = pc.PAIR_PLACES[place]
    pipe = Pipe(pc.PAIR_M, pc.PAIR_M, route)
    accs = [pipe.acc(pc.pair_world(c, place)) for c in PAIRS]
    pipe.close()
    check_pairs(f"{route}, {place}", [a[ia] for a in accs], [a[ib] for a in accs])


@pytest.mark.parametrize("place", list(pc.PAIR_PLACES))
def test_massive_receivers_in_the_potential_and_the_ensembles(place):
    """potential(): the pair inside one tile of 128 runs the masked statement, in two tiles the unmasked one; the ensemble's
    step and SimBatch.potential() on the same worlds."""
    ia, ib = pc.PAIR_PLACES[place]
    worlds = [pc.pair_world(c, place) for c in PAIRS]
    sim = nb.SimPipeline(pc.PAIR_M, pc.PAIR_M)
    phis = []
    for w in worlds:
        sim.set_data(w)
        phis.append(sim.potential())
    sim.close()
    b = nb.SimBatch(pc.PAIR_M, [pc.PAIR_M] * len(worlds))
    b.set_data(np.stack(worlds))
    bphi = b.potential()
    b.update(1, 0.0)
    got = b.get_data()
    b.close()
    check_pairs(f"SimBatch + SimBatch.potential(), {place}", list(got[:, ia, 4:6]), list(got[:, ib, 4:6]), bphi[:, ia], bphi[:, ib])
    check_pairs(f"potential(), {place}", list(got[:, ia, 4:6]), list(got[:, ib, 4:6]), [p[ia] for p in phis], [p[ib] for p in phis])
    same_bits("SimBatch.potential() against potential()", bphi[:, [ia, ib]], np.stack(phis)[:, [ia, ib]])
