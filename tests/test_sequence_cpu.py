"""The sequence driver has teeth (no GPU): tests/sequence_driver.py runs a numpy stand-in for SimPipeline that keeps the same
kinds of state between calls as the real one -- two position buffers and a phase bit, a step size in "device memory" with a
validity flag, a cached chain per phase that remembers the step size it was captured with, an adaptive head, async work that
later calls queue behind, grow-only scratch -- and in which each way of getting that state wrong can be switched on.  Without
a fault every committed seed passes; with each fault at least one committed seed fails, and the driver names an operation at
or after the first one the fault could touch.  The seeds are the ones tests/test_gpu_sequences.py runs on the MI355X."""
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

    def get_data(self):
        self._flush()
        return np.concatenate([self.pos[self.cur], self.vel, self.acc, self.mass[:, None], self.radius[:, None]], axis=1).astype(F32)

    def sync(self):
        self._flush()

    def _latest(self):
        """the positions a reading call works on"""
        if self.fault != 6:
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

    def update(self, n, dt):
        self._flush()
        self._fixed(n, dt)

    def step_async(self, n, dt):
        self.queue.append(lambda: self._fixed(n, dt))

    def _criterion(self, eta, dt_max):
        a2 = (self.acc.astype(np.float64) ** 2).sum(axis=1).astype(F32)
        ok = (a2 > 0) & np.isfinite(a2)
        q = F32(np.min(np.where(self.radius[ok] > 0, self.radius[ok], 0) / a2[ok])) if ok.any() else F32(np.inf)
        if not self.armed:
            self.head_min, self.armed = F32(np.inf), True
        self.head_min = min(self.head_min, q)
        return F32(min(F32(eta) * np.sqrt(np.sqrt(self.head_min, dtype=F32), dtype=F32), F32(dt_max)))

    def _adaptive(self, n, eta, dt_max, span, prime):
        if prime:
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
            log[i] = self.dt_dev = dt          # the device writes the step size where the step reads it
            self._step(dt)
        res["elapsed"] = t
        if self.fault != 1:
            self.dt_valid = False
        self.collected = (log, res)

    def update_adaptive(self, n, eta, dt_max, span=float("inf"), prime=False):
        self._flush()
        self._adaptive(n, eta, dt_max, span, prime)
        return self.collected

    def update_adaptive_async(self, n, eta, dt_max, span=float("inf"), prime=False):
        self.queue.append(lambda: self._adaptive(n, eta, dt_max, span, prime))

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


def view(w, h):
    return types.SimpleNamespace(target=(0.0, 0.0), offset=(w / 2, h / 2), zoom=w / 300.0, width=w, height=h, core_mass=1000.0)


_points = np.random.default_rng(5).standard_normal((max(sd.POINT_COUNTS), 2)).astype(F32) * 60
ENV = sd.Env("pipeline", world(1), world(2), view, lambda k: _points[:k])


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
    return names.index("energy")


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
