"""The sequence driver has teeth (no GPU): tests/sequence_driver.py runs a numpy stand-in for SimPipeline that keeps the same
kinds of state between calls as the real one -- two position buffers and a phase bit, a step size in "device memory" with a
validity flag, a cached chain per phase that remembers the step size it was captured with, an adaptive head, async work that
later calls queue behind, grow-only scratch -- and in which each way of getting that state wrong can be switched on.  Without
a fault every committed seed passes; with each fault at least one committed seed fails, and the driver names an operation at
or after the first one the fault could touch.  The seeds are the ones tests/test_gpu_sequences.py runs on the MI355X.

The leapfrog kinds ("pipeline-lf", "batch-lf"): the stand-in also makes the kick-drift-kick steps of tests/leapfrog_ref.py
around its own force, with two kick words in a head that regrows, a host-side "acc is current" flag, the step word at 0 for
the whole call and last_leapfrog_info(); FakeBatch puts a list of them behind the SimBatch names.  HOW THE SEEDS OF THESE
KINDS WERE CHOSEN (sequence_driver.SEEDS): among the seeds from 0 up whose sequence generates (assert_covers holds) and
passes on the clean stand-in, the first pair in lexicographic order that between them (a) fail every fault of LF_FAULTS that
the kind can show and (b) issue every operation the kind draws and every drawn form of the adaptive calls
(sequence_driver.assert_union_covers, at the member counts of the GPU rows) -- test_the_leapfrog_seeds_are_the_first_pair_that_catches_every_fault recomputes it."""
import hashlib
import itertools
import types

import numpy as np
import pytest

import sequence_driver as sd

F32 = np.float32
N, M = 24, 13

FAULTS = {
    1: "after adaptive steps the next fixed-step call reuses the stale step size (dt_valid not cleared)",
    2: "a diagnostic, render or field call reads pos[cur ^ 1]",
    3: "the cached chain of phase 1 keeps the step size it was captured with",
    4: "a scratch buffer that regrew returns the old, shorter contents for the tail",
    5: "set_data leaves the adaptive head armed: the next criterion starts from the old minimum",
    6: "a diagnostic behind an async step sees the state before the step",
    7: "potential() after energy() returns the previous call's buffer",
}
LF_FAULTS = {
    8: "an Euler update leaves acc_current set",
    9: "set_data leaves acc_current set",
    10: "an Euler adaptive call leaves acc_current set",
    11: "trace leaves acc_current set (FakeBatch)",
    12: "after a leapfrog call the next fixed-step call with an already-used step size steps with the word still at 0",
    13: "an adaptive leapfrog call of odd n closes its last step with the wrong kick-word row",
    14: "a regrown head loses the kick words",
    15: "an async leapfrog call is not waited for by the diagnostic behind it",
    16: "a leapfrog call primes every time (bits cannot show it: only the info oracle can)",
}
LF_FAULTS_OF = {"pipeline-lf": (8, 9, 10, 12, 13, 14, 15, 16), "batch-lf": (8, 9, 10, 11, 12, 13, 16)}
HEAD_LOG = 64          # the step sizes the adaptive head logs before it regrows


def world(seed):
    rng = np.random.default_rng(seed)
    a = np.zeros((N, 8), dtype=F32)
    a[:, 0:2] = rng.standard_normal((N, 2)) * 50
    a[:, 2:4] = rng.standard_normal((N, 2))
    a[:M, 7] = 1.5 + 3 * rng.random(M)
    a[M:, 7] = 0.5
    a[:M, 6] = 40 * a[:M, 7] ** 3
    return a


class FakePipeline:
    """float32 Euler steps with the method names of nb.SimPipeline; `fault` plants one entry of FAULTS."""

    def __init__(self, n, m, fault=0):
        self.n, self.m, self.fault = n, m, fault
        self.pos = [np.zeros((n, 2), F32), np.zeros((n, 2), F32)]
        self.cur = 0
        self.vel, self.acc = np.zeros((n, 2), F32), np.zeros((n, 2), F32)
        self.mass, self.radius = np.zeros(n, F32), np.zeros(n, F32)
        self.dt_dev, self.dt_host, self.dt_valid = F32(0), None, False   # the step size the "kernels" read, and what the host believes
        self.chain = [None, None]                                        # per phase: the step size the cached chain was captured with
        self.head_min, self.armed = F32(np.inf), False                   # the adaptive head
        self.queue = []                                                  # async work that has not run yet
        self.scratch = np.zeros(0, F32)                                  # grow-only, shared by the field calls
        self.phi, self.phi_fresh = None, False
        self.collected = None
        # leapfrog: two kick words in the adaptive head (which regrows), what the host believes word 0 to hold, whether acc
        # is F(x) of the latest state (host side, decided when a call is issued), the record of the last leapfrog call
        self.kick, self.kick_host, self.head_room = np.zeros(2, F32), None, HEAD_LOG
        self.acc_current, self.lf_info = False, (0, False)

    def close(self):
        pass

    # -- state -----------------------------------------------------------------------------------------------------------
    def _flush(self):
        while self.queue:
            self.queue.pop(0)()

    def set_data(self, a):
        self._flush()
        a = np.asarray(a, dtype=F32)
        self.cur = 0
        self.pos[0], self.vel, self.acc = a[:, 0:2].copy(), a[:, 2:4].copy(), a[:, 4:6].copy()
        self.mass, self.radius = a[:, 6].copy(), a[:, 7].copy()
        if self.fault != 5:
            self.armed = False
        if self.fault != 9:
            self.acc_current = False

    def get_data(self):
        self._flush()
        return np.concatenate([self.pos[self.cur], self.vel, self.acc, self.mass[:, None], self.radius[:, None]], axis=1).astype(F32)

    def sync(self):
        self._flush()

    def _latest(self):
        """the positions a reading call works on"""
        behind_leapfrog = self.fault == 15 and self.queue and getattr(self.queue[-1], "leapfrog", False)
        if self.fault != 6 and not behind_leapfrog:
            self._flush()
        return self.pos[self.cur ^ 1] if self.fault == 2 else self.pos[self.cur]

    # -- steps -----------------------------------------------------------------------------------------------------------
    def _force(self, p):
        d = p[None, :self.m, :] - p[:, None, :]
        r2 = (d * d).sum(axis=2) + self.radius[:, None]
        return (d * (self.mass[None, :self.m] / (r2 * np.sqrt(r2)))[:, :, None]).sum(axis=1).astype(F32)

    def _step(self, dt):
        p = self.pos[self.cur]
        self.acc = self._force(p)
        self.vel = self.vel + self.acc * F32(dt)
        self.pos[self.cur ^ 1] = p + self.vel * F32(dt)
        self.cur ^= 1
        self.armed = False          # the state moved: the head's minimum is no longer this state's

    def _fixed(self, n, dt):
        dt = F32(dt)
        if not self.dt_valid or self.dt_host != dt:          # upload only a step size the device does not hold
            self.dt_dev, self.dt_host, self.dt_valid = dt, dt, True
        use = self.dt_dev
        if n >= 2:                                           # a chain, cached per phase, reads the step size from device memory
            if self.chain[self.cur] is None:
                self.chain[self.cur] = self.dt_dev
            if self.fault == 3 and self.cur == 1:
                use = self.chain[1]
        for _ in range(n):
            self._step(use)

    def _issued(self, leapfrog):
        """host side, when a stepping call is issued: does it prime, and what it leaves of acc_current"""
        primed = leapfrog and (not self.acc_current or self.fault == 16)
        self.acc_current = leapfrog
        return primed

    def update(self, n, dt):
        self._flush()
        if self.fault != 8:
            self._issued(False)
        self._fixed(n, dt)

    def step_async(self, n, dt):
        if self.fault != 8:
            self._issued(False)
        self.queue.append(lambda: self._fixed(n, dt))

    # -- leapfrog (tests/leapfrog_ref.py: open, force, close; nothing merged) ---------------------------------------------
    def _grow_head(self, log):
        if log > self.head_room:
            self.head_room = log
            if self.fault == 14:
                self.kick = np.zeros(2, F32)         # the new buffer; the host goes on believing what it uploaded

    def _kick(self, row):
        self.vel = self.vel + self.acc * (F32(0.5) * self.kick[row])

    def _open(self, row):
        self._kick(row)
        self.pos[self.cur] = self.pos[self.cur] + self.vel * self.kick[row]          # the drift, in place

    def _begin_leapfrog(self, primed):
        self.dt_dev = F32(0)                  # the step word: every launch of the call is a force evaluation
        if primed:
            self._step(self.dt_dev)

    def _end_leapfrog(self):
        if self.fault != 12:
            self.dt_valid = False

    def _leapfrog(self, n, dt, primed):
        self._grow_head(0)
        dt = F32(dt)
        if self.kick_host != dt:
            self.kick[0], self.kick_host = dt, dt
        self._begin_leapfrog(primed)
        for i in range(n):
            if i > 0:
                self._kick(0)
            self._open(0)
            self._step(self.dt_dev)
        self._kick(0)
        self._end_leapfrog()

    def update_leapfrog(self, n, dt):
        self._flush()
        primed = self._issued(True)
        self.lf_info = (n + primed, primed)
        self._leapfrog(n, dt, primed)

    def update_leapfrog_async(self, n, dt):
        primed = self._issued(True)
        self.lf_info = (n + primed, primed)
        work = lambda: self._leapfrog(n, dt, primed)          # noqa: E731
        work.leapfrog = True
        self.queue.append(work)

    def last_leapfrog_info(self):
        return self.lf_info

    def _criterion(self, eta, dt_max):
        a2 = (self.acc.astype(np.float64) ** 2).sum(axis=1).astype(F32)
        ok = (a2 > 0) & np.isfinite(a2)
        q = F32(np.min(np.where(self.radius[ok] > 0, self.radius[ok], 0) / a2[ok])) if ok.any() else F32(np.inf)
        if not self.armed:
            self.head_min, self.armed = F32(np.inf), True
        self.head_min = min(self.head_min, q)
        return F32(min(F32(eta) * np.sqrt(np.sqrt(self.head_min, dtype=F32), dtype=F32), F32(dt_max)))

    def _adaptive(self, n, eta, dt_max, span, prime, leapfrog=False, primed=False):
        self._grow_head(n)
        if leapfrog:
            self.kick_host = None             # the criterion writes the kick words
            self._begin_leapfrog(primed)
        elif prime:
            self._step(0.0)
        t, log, res = 0.0, np.zeros(n, F32), dict(elapsed=0.0, steps=0, idle_steps=0, dt_last=0.0, dt_smallest=0.0)
        for i in range(n):
            dt = self._criterion(eta, dt_max)
            if span - t <= 0:
                dt = F32(0)
            elif float(dt) >= span - t:
                dt, t = F32(span - t), span
            else:
                t += float(dt)
            if dt > 0:
                res["steps"] += 1
                res["dt_last"] = float(dt)
                res["dt_smallest"] = float(dt) if res["dt_smallest"] == 0 else min(res["dt_smallest"], float(dt))
            else:
                res["idle_steps"] += 1
            if leapfrog:                       # the device writes the step size into kick word i & 1
                row = i & 1
                log[i] = self.kick[row] = dt
                if i > 0:
                    self._kick(row ^ 1)
                self._open(row)
                self._step(self.dt_dev)
                continue
            log[i] = self.dt_dev = dt          # the device writes the step size where the step reads it
            self._step(dt)
        res["elapsed"] = t
        if leapfrog:
            last = (n - 1) & 1
            self._kick(last ^ 1 if self.fault == 13 and n % 2 == 1 else last)
            self._end_leapfrog()
        elif self.fault != 1:
            self.dt_valid = False
        self.collected = (log, res)

    def _issued_adaptive(self, leapfrog):
        if leapfrog or self.fault != 10:
            primed = self._issued(leapfrog)
        else:
            primed = False
        return primed

    def update_adaptive(self, n, eta, dt_max, span=float("inf"), prime=False, leapfrog=False):
        self._flush()
        primed = self._issued_adaptive(leapfrog)
        if leapfrog:
            self.lf_info = (n + primed, primed)
        self._adaptive(n, eta, dt_max, span, prime, leapfrog, primed)
        return self.collected

    def update_adaptive_async(self, n, eta, dt_max, span=float("inf"), prime=False, leapfrog=False):
        primed = self._issued_adaptive(leapfrog)
        if leapfrog:
            self.lf_info = (n + primed, primed)
        work = lambda: self._adaptive(n, eta, dt_max, span, prime, leapfrog, primed)          # noqa: E731
        work.leapfrog = leapfrog
        self.queue.append(work)

    def adaptive_collect(self, n):
        self._flush()
        return self.collected

    def timestep(self, eta, dt_max):
        self._flush()
        return float(self._criterion(eta, dt_max))

    # -- reading calls ---------------------------------------------------------------------------------------------------
    def _phi(self, p, at, soft):
        d = p[None, :self.m, :].astype(np.float64) - at[:, None, :]
        return -(self.mass[None, :self.m] / np.sqrt((d * d).sum(axis=2) + soft)).sum(axis=1)

    def energy(self):
        p = self._latest().astype(np.float64)
        self.phi, self.phi_fresh = self._phi(p, p, 1.0).astype(F32), True
        mass, v = self.mass.astype(np.float64), self.vel.astype(np.float64)
        mom = (mass[:, None] * v).sum(axis=0)
        com = (mass[:, None] * p).sum(axis=0) / mass.sum()
        return {"kinetic": float(0.5 * (mass * (v * v).sum(axis=1)).sum()), "potential": float(0.5 * (mass * self.phi).sum()),
                "mass": float(mass.sum()), "momentum": (float(mom[0]), float(mom[1])),
                "angular_momentum": float((mass * (p[:, 0] * v[:, 1] - p[:, 1] * v[:, 0])).sum()),
                "center_of_mass": (float(com[0]), float(com[1]))}

    def potential(self):
        p = self._latest().astype(np.float64)
        if not (self.fault == 7 and self.phi_fresh):
            self.phi = self._phi(p, p, 1.0).astype(F32)
        self.phi_fresh = False
        return self.phi.copy()

    def _into_scratch(self, values):
        """the result travels through the scratch buffer, which grows when a call needs more"""
        had = self.scratch.size
        if had < values.size:
            self.scratch = np.zeros(values.size, F32)
        count = had if (self.fault == 4 and 0 < had < values.size) else values.size
        self.scratch[:count] = values[:count]
        return self.scratch[:values.size].copy()

    def potential_at(self, points, soft):
        p = self._latest().astype(np.float64)
        return self._into_scratch(self._phi(p, np.asarray(points, np.float64), soft).astype(F32))

    def acceleration_at(self, points, soft):
        p, at = self._latest().astype(np.float64), np.asarray(points, np.float64)
        d = p[None, :self.m, :] - at[:, None, :]
        r2 = (d * d).sum(axis=2) + soft
        g = (d * (self.mass[None, :self.m] / (r2 * np.sqrt(r2)))[:, :, None]).sum(axis=1).astype(F32)
        return self._into_scratch(g.reshape(-1)).reshape(-1, 2)

    @staticmethod
    def _pixels(view):
        ys, xs = np.mgrid[0:view.height, 0:view.width]
        return np.stack([(xs.reshape(-1) + 0.5 - view.offset[0]) / view.zoom + view.target[0],
                         (ys.reshape(-1) + 0.5 - view.offset[1]) / view.zoom + view.target[1]], axis=1)

    def potential_map(self, view, soft):
        return self.potential_at(self._pixels(view), soft).reshape(view.height, view.width)

    def acceleration_map(self, view, soft):
        return self.acceleration_at(self._pixels(view), soft).reshape(view.height, view.width, 2)

    def bounds(self):
        p = self._latest()
        return np.concatenate([p.min(axis=0), p.max(axis=0)]).astype(F32)

    def render_counts(self, view):
        p = self._latest()
        s = (p - np.asarray(view.target, F32)) * F32(view.zoom) + np.asarray(view.offset, F32)
        out = np.zeros((3, view.height, view.width), np.uint32)
        ok = (s[:, 0] >= 0) & (s[:, 0] < view.width) & (s[:, 1] >= 0) & (s[:, 1] < view.height)
        cls = np.where(self.mass <= 0, 0, np.where(self.mass < view.core_mass, 1, 2))
        np.add.at(out, (cls[ok], s[ok, 1].astype(np.int64), s[ok, 0].astype(np.int64)), 1)
        return out

    def render(self, view):
        c = self.render_counts(view)
        return np.minimum(c.transpose(1, 2, 0) * 80, 255).astype(np.uint8)


class FakeBatch:
    """A list of FakePipeline members behind the method names of nb.SimBatch that the driver calls; step sizes one for all
    or one per member; trace records energy() rows."""

    def __init__(self, count, n, m, fault=0):
        self.members, self.fault = [FakePipeline(n, m, fault) for _ in range(count)], fault

    def close(self):
        pass

    def _dts(self, dt):
        return [float(dt)] * len(self.members) if np.ndim(dt) == 0 else [float(x) for x in dt]

    def set_data(self, a):
        for s, part in zip(self.members, a):
            s.set_data(part)

    def get_data(self):
        return np.stack([s.get_data() for s in self.members])

    def get_member(self, b):
        return self.members[b].get_data()

    def update(self, n, dt):
        for s, d in zip(self.members, self._dts(dt)):
            s.update(n, d)

    def step_async(self, n, dts):
        for s, d in zip(self.members, self._dts(dts)):
            s.step_async(n, d)

    def update_leapfrog(self, n, dt):
        for s, d in zip(self.members, self._dts(dt)):
            s.update_leapfrog(n, d)

    def last_leapfrog_info(self):
        return self.members[0].last_leapfrog_info()

    def update_adaptive(self, n, eta, dt_max, span=float("inf"), prime=False, leapfrog=False):
        outs = [s.update_adaptive(n, eta, dt_max, span, prime, leapfrog) for s in self.members]
        return np.stack([log for log, _ in outs], axis=1), [res for _, res in outs]

    def trace(self, n, dt, every):
        def row():
            return [np.frombuffer(sd.ebits(s.energy()), dtype=np.float64) for s in self.members]
        current = [s.acc_current for s in self.members]
        rows = [row()]
        for k in range(n):
            self.update(1, dt)
            if (k + 1) % every == 0:
                rows.append(row())
        if self.fault == 11:
            for s, c in zip(self.members, current):
                s.acc_current = c
        return np.array(rows)

    def energy(self):
        return [s.energy() for s in self.members]

    def potential(self):
        return np.stack([s.potential() for s in self.members])

    def bounds(self):
        return np.stack([s.bounds() for s in self.members])

    def render_mode(self, mode):
        self.mode = mode

    def render_counts(self, view):
        return np.stack([s.render_counts(view) for s in self.members])

    def render(self, view):
        return np.stack([s.render(view) for s in self.members])


def view(w, h):
    return types.SimpleNamespace(target=(0.0, 0.0), offset=(w / 2, h / 2), zoom=w / 300.0, width=w, height=h, core_mass=1000.0)


_points = np.random.default_rng(5).standard_normal((max(sd.POINT_COUNTS), 2)).astype(F32) * 60
ENV = sd.Env("pipeline", world(1), world(2), view, lambda k: _points[:k])
B = 3
LF_ENVS = {"pipeline-lf": sd.Env("pipeline-lf", world(1), world(2), view, lambda k: _points[:k]),
           "batch-lf": sd.Env("batch-lf", np.stack([world(10 + b) for b in range(B)]), np.stack([world(20 + b) for b in range(B)]),
                              view, None, members=B)}
for _env in LF_ENVS.values():
    sd.assert_premise(_env.start, _env.other)          # the premise of the leapfrog kinds, for the stand-in's states


def lf_maker(kind, fault=0):
    if kind == "pipeline-lf":
        return lambda: FakePipeline(N, M, fault)
    return lambda: FakeBatch(B, N, M, fault)


def first_touch(fault, ops):
    """index of the first operation the fault could change the output of"""
    names = [name for name, _ in ops]

    def first(pred, start=0):
        return next(i for i in range(start, len(ops)) if pred(*ops[i]))
    if fault == 1:
        return first(lambda n, a: n in ("update", "step_async"), first(lambda n, a: n in sd.ADAPTIVE) + 1)
    if fault == 2:
        return first(lambda n, a: n in sd.DIAGNOSTICS)
    if fault == 3:
        return first(lambda n, a: n in ("update", "step_async") and a["n"] >= 2)
    if fault == 4:
        return first(lambda n, a: n in ("potential_at", "acceleration_at", "potential_map", "acceleration_map"))
    if fault == 5:
        return names.index("set_data")
    if fault == 6:
        return first(lambda n, a: n in sd.ASYNC)
    if fault == 7:
        return names.index("energy")
    lf = first(lambda n, a: sd.is_leapfrog((n, a)))          # nothing of LF_FAULTS shows before the first leapfrog call
    if fault == 8:
        return first(lambda n, a: n in ("update", "step_async"), lf + 1)
    if fault == 9:
        return first(lambda n, a: n == "set_data", lf + 1)
    if fault == 10:
        return first(lambda n, a: n in sd.ADAPTIVE and not a.get("leapfrog"), lf + 1)
    if fault == 11:
        return first(lambda n, a: n == "trace", lf + 1)
    if fault == 12:
        return first(lambda n, a: n in sd.FIXED, lf + 1)
    if fault == 13:
        return first(lambda n, a: n in sd.ADAPTIVE and a.get("leapfrog") and a["n"] % 2 == 1)
    if fault == 14:
        return first(lambda n, a: n in sd.ADAPTIVE and a["n"] > HEAD_LOG)
    if fault == 15:
        return first(lambda n, a: n == "update_leapfrog_async")
    return lf + 1          # 16: the first call primes by right


@pytest.mark.parametrize("seed", sd.SEEDS["pipeline"])
def test_without_a_fault_every_committed_seed_passes(seed):
    ops = sd.generate("pipeline", seed)
    compared = sd.check(lambda: FakePipeline(N, M), ops, ENV, seed)
    assert compared > len(ops) // 2          # most operations return something to compare


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_every_planted_fault_is_caught_by_a_committed_seed(fault):
    caught = []
    for seed in sd.SEEDS["pipeline"]:
        ops = sd.generate("pipeline", seed)
        try:
            sd.check(lambda: FakePipeline(N, M, fault), ops, ENV, seed)
        except sd.SequenceMismatch as e:
            assert e.seed == seed and e.index >= first_touch(fault, ops), (FAULTS[fault], e.index, first_touch(fault, ops))
            assert e.name == (ops[e.index][0] if e.index < len(ops) else "final state")
            assert f"seed {seed}" in str(e) and f"operation {e.index} " in str(e) and sd.show(ops[0]) in str(e)
            caught.append(seed)
    assert caught, f"no committed seed notices: {FAULTS[fault]}"


@pytest.mark.parametrize("kind,members", [("pipeline", 0), ("batch", 5), ("batch", 3), ("ragged", 12)])
def test_committed_sequences_hold_what_they_must(kind, members):
    for seed in sd.SEEDS[kind]:
        ops = sd.generate(kind, seed, members=members)
        sd.assert_covers(kind, ops)
        assert sd.LENGTH <= len(ops) <= sd.LENGTH + 4
        assert ops == sd.generate(kind, seed, members=members)          # a seed names one sequence
        if kind == "ragged":
            assert {name for name, _ in ops} <= sd.RAGGED_ALLOWED


def test_the_generator_notices_a_dropped_requirement():
    ops = sd.generate("pipeline", sd.SEEDS["pipeline"][0])
    with pytest.raises(AssertionError, match="set_data"):
        sd.assert_covers("pipeline", [op for op in ops if op[0] != "set_data"])
    with pytest.raises(AssertionError, match="async"):
        sd.assert_covers("pipeline", [op for op in ops if op[0] not in sd.ASYNC and op[0] != "adaptive_collect"])
    with pytest.raises(AssertionError):
        sd.assert_covers("ragged", ops)


# ---- the leapfrog kinds ---------------------------------------------------------------------------------------------------------

def lf_members(kind):
    return B if kind == "batch-lf" else 0


def caught_by(kind, seed, fault):
    """None: the sequence passes; else the SequenceMismatch"""
    ops = sd.generate(kind, seed, members=lf_members(kind))
    try:
        sd.check(lf_maker(kind, fault), ops, LF_ENVS[kind], seed)
    except sd.SequenceMismatch as e:
        return e
    return None


@pytest.mark.parametrize("kind", sorted(LF_FAULTS_OF))
def test_without_a_fault_every_committed_leapfrog_seed_passes(kind):
    for seed in sd.SEEDS[kind]:
        ops = sd.generate(kind, seed, members=lf_members(kind))
        assert sd.check(lf_maker(kind), ops, LF_ENVS[kind], seed) > len(ops) // 2


@pytest.mark.parametrize("kind,fault", [(k, f) for k in sorted(LF_FAULTS_OF) for f in LF_FAULTS_OF[k]])
def test_every_planted_leapfrog_fault_is_caught_by_a_committed_seed(kind, fault):
    caught = []
    for seed in sd.SEEDS[kind]:
        e = caught_by(kind, seed, fault)
        if e is not None:
            ops = sd.generate(kind, seed, members=lf_members(kind))
            assert e.seed == seed and e.index >= first_touch(fault, ops), (LF_FAULTS[fault], e.index, first_touch(fault, ops))
            assert e.name == (ops[e.index][0] if e.index < len(ops) else "final state")
            assert f"seed {seed}" in str(e) and sd.show(ops[0]) in str(e)
            if fault == 16:
                assert "last_leapfrog_info" in str(e)          # the bits agree: only the second oracle sees it
            caught.append(seed)
    assert caught, f"no committed seed of {kind} notices: {LF_FAULTS[fault]}"


@pytest.mark.parametrize("kind", sorted(LF_FAULTS_OF))
def test_the_leapfrog_seeds_are_the_first_pair_that_catches_every_fault(kind):
    """The rule of the module docstring, recomputed; candidates that do not generate or do not pass clean are left out."""
    catches = {}
    for seed in range(max(sd.SEEDS[kind]) + 1):
        try:
            if caught_by(kind, seed, 0) is None:
                catches[seed] = {f for f in LF_FAULTS_OF[kind] if caught_by(kind, seed, f) is not None}
        except AssertionError:
            continue          # assert_covers: this seed names no sequence

    def good(pair):
        if catches[pair[0]] | catches[pair[1]] != set(LF_FAULTS_OF[kind]):
            return False
        try:
            for members in UNION_MEMBERS[kind]:          # the member counts of the GPU rows: get_member draws depend on them
                sd.assert_union_covers(kind, [sd.generate(kind, seed, members=members) for seed in pair])
        except AssertionError:
            return False
        return True
    pairs = (p for p in itertools.combinations(sorted(catches), 2) if good(p))
    assert next(pairs) == tuple(sd.SEEDS[kind]), {s: sorted(c) for s, c in catches.items()}


UNION_MEMBERS = {"pipeline-lf": (0,), "batch-lf": (3, 5)}


@pytest.mark.parametrize("kind,members", [(k, m) for k in sorted(UNION_MEMBERS) for m in UNION_MEMBERS[k]])
def test_the_committed_leapfrog_sequences_issue_every_operation_between_them(kind, members):
    """at the member counts the GPU rows run, too (get_member draws depend on them)"""
    sd.assert_union_covers(kind, [sd.generate(kind, seed, members=members) for seed in sd.SEEDS[kind]])


@pytest.mark.parametrize("kind", sorted(LF_FAULTS_OF))
def test_committed_leapfrog_sequences_hold_what_they_must(kind):
    for seed in sd.SEEDS[kind]:
        ops = sd.generate(kind, seed, members=lf_members(kind))
        sd.assert_covers(kind, ops)
        assert sd.LF_LENGTH <= len(ops) <= sd.LF_LENGTH + 4
        assert ops == sd.generate(kind, seed, members=lf_members(kind))
        assert not any(a.get("resume") for _, a in ops)
        if kind == "batch-lf":
            assert not any(name == "update_leapfrog_async" for name, _ in ops)


def test_the_generator_notices_a_dropped_leapfrog_piece():
    ops = sd.generate("batch-lf", sd.SEEDS["batch-lf"][0], members=B)
    with pytest.raises(AssertionError, match="trace"):
        sd.assert_covers("batch-lf", [op for op in ops if op[0] != "trace"])
    ops = sd.generate("pipeline-lf", sd.SEEDS["pipeline-lf"][0])
    with pytest.raises(AssertionError, match="64"):
        sd.assert_covers("pipeline-lf", [op for op in ops if not (op[0] in sd.ADAPTIVE and op[1]["n"] > 64)])
    with pytest.raises(AssertionError, match="update_leapfrog_async"):
        sd.assert_covers("pipeline-lf", [op for op in ops if op[0] != "update_leapfrog_async"])
    with pytest.raises(AssertionError, match="in a row"):
        sd.assert_covers("pipeline-lf", [op for i, op in enumerate(ops) if not (i and sd.is_leapfrog(op) and sd.is_leapfrog(ops[i - 1]))])


def test_the_premise_is_asserted():
    bad = world(1)
    bad[3, 2] = -0.0
    with pytest.raises(AssertionError, match="-0.0"):
        sd.assert_premise(bad)
    bad[3, 2] = np.inf
    with pytest.raises(AssertionError, match="finite"):
        sd.assert_premise(bad)


# generate(kind, seed) of the kinds that existed before the leapfrog kinds, as sha256 of repr(ops): those sequences are what
# the GPU rows of these kinds have always run, and new code paths of the generator must not move them
OLD_SEQUENCES = {
    ("pipeline", 0, 5): "dda975947a605c1d9a64bb1f74159cf6ac82039916466a8851c1b036f369a700",
    ("pipeline", 0, 8): "8e6dc8b354dca0e4d81e8316ec1e10e96d047428d76b6c2a1137d32479920d5a",
    ("pipeline", 0, 11): "cf84664908413741d250d581635a96b7336c3de444a54b1597ebea88d48c27b0",
    ("batch", 5, 5): "23c9cd156ddf97a3e5f1ade6ad7412023b2b4b4587d484871cc17bd15d906888",
    ("batch", 5, 8): "5552582e06e4823bf216d0564d155efb0ed080a28640610b5bb53ccd25861410",
    ("batch", 3, 5): "edb86b33734249bd61b723093418b409ee493cd51ea69cba3fc4a3bb389ca095",
    ("batch", 3, 8): "5552582e06e4823bf216d0564d155efb0ed080a28640610b5bb53ccd25861410",
    ("ragged", 12, 5): "04a2856e26e0b414a5f1698a4d8c67eb47b96dfacf93140c895f82303cd2495a",
    ("ragged", 12, 8): "e13dfd1687918aa805171449ab74d2b5b1f8917d6615d5d49b19da90e993437d",
}


@pytest.mark.parametrize("kind,members,seed", sorted(OLD_SEQUENCES))
def test_the_sequences_of_the_old_kinds_have_not_moved(kind, members, seed):
    ops = sd.generate(kind, seed, members=members)
    assert hashlib.sha256(repr(ops).encode()).hexdigest() == OLD_SEQUENCES[(kind, members, seed)]
    assert not any(sd.is_leapfrog(op) or op[0] in sd.LEAPFROG for op in ops)
