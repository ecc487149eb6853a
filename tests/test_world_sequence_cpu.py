"""The World sequence driver (tests/world_sequence.py) without a GPU, twice.

1. Against the real libnbody.so: the World kind restricted to the operations that cannot reach a device (update_cpu,
   update_cpu_leapfrog, update_cpu_adaptive, timestep, particles, every diagnostic, the renders), same driver, same seeds, at
   N = 200 and 600; a child process runs them all again and is then held to having opened no device.

2. Teeth: a numpy FakeWorld / FakeWorldBatch with a host array, a device copy, the flags of world.c / world_batch.c and two
   diagnostic paths that differ in bits by construction (the device path scales by 1 + 2^-10 in float32; the device's force
   differs from the host's in the same way, so an acc that crossed sides is not the other side's own).  Each way of getting
   the coherence wrong can be switched on.  Without a fault every committed seed passes; with each fault at least one
   committed seed of the kind fails, at or after the first operation the fault could touch.

HOW THE SEEDS WERE CHOSEN (world_sequence.SEEDS): among the seeds from 0 up whose sequence generates and passes on the clean
stand-in, the first pair in lexicographic order that between them (a) fail every fault the kind can show and (b) issue every
operation the kind draws and every drawn form of the adaptive calls (world_sequence.assert_union_covers, at the member counts
the GPU rows run with); test_the_seeds_are_the_first_pair_that_catches_every_fault recomputes that choice.

The reads kinds: against the real library the CPU-only run also drives the host paths of tidal_at, tidal_map, profile, pair_counts
and neighbours in long sequences; the stand-in answers the tidal calls in its two arithmetics and the three exact calls the same on
either side (tests/paircount_ref.py, tests/neighbour_ref.py), and has two more faults: a new read answered by the side that is not
the newest (11), and a new read that flips device_is_newer (12)."""
import itertools
import types

import numpy as np
import pytest

import nbody_amd as nb
import neighbour_ref as nref
import paircount_ref as pref
import reads_common
import sequence_driver as sd
import world_sequence as ws
from gpu_common import synth
from test_leapfrog_cpu import child
from test_sequence_cpu import MASK_OF, read_centre, read_edges, read_points, read_view, sample

F32, F64 = np.float32, np.float64
SKEW = F32(1 + 2.0 ** -10)          # what tells the device's arithmetic from the host's

FAULTS = {
    1: "a CPU step does not pull",
    2: "a CPU step does not mark the host newer",
    3: "a GPU step does not push (after the object's first upload: a fresh object with this fault would fail every test)",
    4: "a diagnostic is answered by the wrong side after a CPU step",
    5: "a diagnostic reads the device while the host is newer",
    6: "particles() leaves cpu_acc_current set after pulling",
    7: "update_cpu leaves cpu_acc_current set",
    8: "an n = 0 GPU call marks the device newer",
    9: "a traced batch update of n > 0 does not mark the device newer",
    10: "a member() read does not refresh the array",
    11: "tidal_at, tidal_map, profile, pair_counts or neighbours answers from the side that is not the newest",
    12: "tidal_at, tidal_map, profile, pair_counts or neighbours flips device_is_newer",
}
# a WorldBatch uploads once in its life (nothing on the host changes the array), so fault 3 has no meaning for it
FAULTS_OF = {"world": (1, 2, 3, 4, 5, 6, 7, 8), "batch": (8, 9, 10), "ragged": (8, 9, 10),
             "world-reads": (1, 2, 3, 4, 5, 6, 7, 8, 11, 12), "batch-reads": (8, 9, 10, 11, 12), "ragged-reads": (8, 9, 10, 11, 12)}


# ---- the physics of the stand-in: float32, one force for the host and a skewed one for the device -------------------------------

def massive(a):
    return int(np.count_nonzero(a[:, 6] > 0))


def euler(a, dt, skew):
    a, m = a.copy(), massive(a)
    p = a[:, 0:2]
    d = p[None, :m, :] - p[:, None, :]
    r2 = (d * d).sum(axis=2) + a[:, 7][:, None]
    acc = (d * (a[None, :m, 6] / (r2 * np.sqrt(r2)))[:, :, None]).sum(axis=1).astype(F32)
    a[:, 4:6] = acc * SKEW if skew else acc
    a[:, 2:4] = a[:, 2:4] + a[:, 4:6] * F32(dt)
    a[:, 0:2] = a[:, 0:2] + a[:, 2:4] * F32(dt)
    return a


def kick(a, dt, drift):
    a = a.copy()
    a[:, 2:4] = a[:, 2:4] + a[:, 4:6] * (F32(0.5) * F32(dt))
    if drift:
        a[:, 0:2] = a[:, 0:2] + a[:, 2:4] * F32(dt)
    return a


def leapfrog_step(a, dt, skew):
    return kick(euler(kick(a, dt, True), 0.0, skew), dt, False)


def criterion(a, eta, dt_max):
    a2 = (a[:, 4:6].astype(F64) ** 2).sum(axis=1).astype(F32)
    ok = (a2 > 0) & np.isfinite(a2)
    q = F32(np.min(a[ok, 7] / a2[ok])) if ok.any() else F32(np.inf)
    return F32(min(F32(eta) * np.sqrt(np.sqrt(q, dtype=F32), dtype=F32), F32(dt_max)))


def adaptive(a, n, eta, dt_max, span, prime, leapfrog, acc_current, skew, stop_at_span=False):
    """(state, log, result) of n device- or host-chosen steps (an advance: until the span is covered)"""
    if n > 0 and ((leapfrog and not acc_current) or (prime and not leapfrog)):
        a = euler(a, 0.0, skew)
    t, log, res = 0.0, [], dict(elapsed=0.0, steps=0, idle_steps=0, dt_last=0.0, dt_smallest=0.0)
    for _ in range(n):
        if stop_at_span and t >= span:
            break
        dt = criterion(a, eta, dt_max)
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
        log.append(dt)
        a = leapfrog_step(a, dt, skew) if leapfrog else euler(a, dt, skew)
    res["elapsed"] = t
    return a, np.array(log, dtype=F32), res


class Reader:
    """Every reading call on one array, in the host's arithmetic or the device's."""

    def __init__(self, a, device):
        self.a, self.m, self.device = a, massive(a), device

    def close(self):
        pass

    def _out(self, x):
        x = np.asarray(x, dtype=F32)
        return x * SKEW if self.device else x

    def _field(self, at, soft):
        d = self.a[None, :self.m, 0:2].astype(F64) - np.asarray(at, F64)[:, None, :]
        r2 = (d * d).sum(axis=2) + np.asarray(soft, F64).reshape(-1, 1)
        mass = self.a[None, :self.m, 6].astype(F64)
        return -(mass / np.sqrt(r2)).sum(axis=1), (d * (mass / (r2 * np.sqrt(r2)))[:, :, None]).sum(axis=1)

    def potential(self):
        return self._out(self._field(self.a[:, 0:2], self.a[:, 7])[0])

    def energy(self):
        a, m = self.a.astype(F64), self.m
        mass, p, v = a[:m, 6], a[:m, 0:2], a[:m, 2:4]
        phi = self.potential().astype(F64)[:m]
        kin = 0.5 * (mass * (v * v).sum(axis=1)).sum()
        mom, com = (mass[:, None] * v).sum(axis=0), (mass[:, None] * p).sum(axis=0) / max(mass.sum(), 1e-300)
        return {"kinetic": float(F32(kin)) if self.device else float(kin), "potential": float(0.5 * (mass * phi).sum()), "mass": float(mass.sum()),
                "momentum": (float(mom[0]), float(mom[1])), "angular_momentum": float((mass * (p[:, 0] * v[:, 1] - p[:, 1] * v[:, 0])).sum()),
                "center_of_mass": (float(com[0]), float(com[1]))}

    def potential_at(self, points, soft):
        return self._out(self._field(points, soft)[0])

    def acceleration_at(self, points, soft):
        return self._out(self._field(points, soft)[1])

    @staticmethod
    def _pixels(view):
        ys, xs = np.mgrid[0:view.height, 0:view.width]
        return np.stack([(xs.reshape(-1) + 0.5 - view.offset[0]) / view.zoom + view.target[0],
                         (ys.reshape(-1) + 0.5 - view.offset[1]) / view.zoom + view.target[1]], axis=1)

    def potential_map(self, view, soft):
        return self.potential_at(self._pixels(view), soft).reshape(view.height, view.width)

    def acceleration_map(self, view, soft):
        return self.acceleration_at(self._pixels(view), soft).reshape(view.height, view.width, 2)

    def tidal_at(self, points, soft):
        return self._out(sample(3, self.a[:self.m, 0:2], self.a[:self.m, 6], np.asarray(points, F32), soft))

    def tidal_map(self, view, soft):
        return self.tidal_at(self._pixels(view), soft).reshape(view.height, view.width, 3)

    # bitwise the same on both paths
    def profile(self, edges, centre, centre_velocity, weights, return_unplaced=False):
        top = self.m if weights == "mass" else self.a.shape[0]
        a = self.a[:top].astype(F64)
        w = a[:, 6] if weights == "mass" else np.ones(top)
        d, u = a[:, 0:2] - np.asarray(centre, F64), a[:, 2:4] - np.asarray(centre_velocity, F64)
        r2 = (d * d).sum(axis=1)
        out = np.zeros((len(edges) + 1, 6))
        row = np.searchsorted(np.asarray(edges, F64), np.sqrt(r2), side="right")
        for col, v in enumerate((np.ones(top), w, w * r2, w * (d[:, 0] * u[:, 1] - d[:, 1] * u[:, 0]), w * (d * u).sum(axis=1),
                                 0.5 * w * (u * u).sum(axis=1))):
            np.add.at(out[:, col], row, v)
        return out, 0

    def pair_counts(self, edges, classes=("mm",), return_unplaced=False):
        mask = sum({"mm": pref.MM, "mt": pref.MT, "tt": pref.TT, "all": pref.ALL}[c] for c in ((classes,) if isinstance(classes, str) else classes))
        return pref.model(self.a, self.m, edges, mask)

    def neighbours(self, radius=None, receivers="all", sources="all"):
        return tuple(x for x in nref.model(self.a, self.m, MASK_OF[receivers], MASK_OF[sources], radius) if x is not None)

    def timestep(self, eta, dt_max):
        return float(criterion(self.a, eta, dt_max))

    def bounds(self):
        p = self.a[:, 0:2]
        return np.concatenate([p.min(axis=0), p.max(axis=0)]).astype(F32)

    def fit_view(self, width, height):
        b = self.bounds()
        return np.array([(b[0] + b[2]) / 2, (b[1] + b[3]) / 2, width / max(float(b[2] - b[0]), 1e-30), width, height], dtype=F32)

    def render_counts(self, view):
        s = (self.a[:, 0:2] - np.asarray(view.target, F32)) * F32(view.zoom) + np.asarray(view.offset, F32)
        out = np.zeros((3, view.height, view.width), np.uint32)
        ok = (s[:, 0] >= 0) & (s[:, 0] < view.width) & (s[:, 1] >= 0) & (s[:, 1] < view.height)
        cls = np.where(self.a[:, 6] <= 0, 0, np.where(self.a[:, 6] < view.core_mass, 1, 2))
        np.add.at(out, (cls[ok], s[ok, 1].astype(np.int64), s[ok, 0].astype(np.int64)), 1)
        return out

    def render(self, view):
        return np.minimum(self.render_counts(view).transpose(1, 2, 0) * 80, 255).astype(np.uint8)


READS = ws.PATH_READS + tuple(n for n in ws.BITWISE_READS if n != "fit_views")


class FakeWorld:
    """world.c in numpy: the array, a device copy, host_is_newer / device_is_newer / cpu_acc_current (and the device's own
    knowledge of its acc); `fault` plants one entry of FAULTS."""

    def __init__(self, particles, fault=0):
        self.h, self.fault = np.array(particles, dtype=F32), fault
        self.d = np.zeros_like(self.h)          # device memory that has seen nothing yet
        self.host_is_newer, self.device_is_newer, self.cpu_acc_current, self.gpu_acc_current, self.pushed = True, False, False, False, False

    def close(self):
        pass

    def _pull(self):
        if self.device_is_newer:
            self.h, self.device_is_newer = self.d.copy(), False
            if self.fault != 6:
                self.cpu_acc_current = False

    def particles(self):
        self._pull()
        return self.h.copy()

    def __getattr__(self, name):
        """the reading calls: on the side the rule names, in that side's arithmetic"""
        if name not in READS:
            raise AttributeError(name)
        on_device = not self.host_is_newer
        a = self.d if on_device else self.h
        if self.host_is_newer and self.pushed:
            if self.fault == 4:
                on_device = True                # the right state, the wrong path
            elif self.fault == 5:
                a, on_device = self.d, True     # the device's older state
        if name in sd.NEW_READS:
            if self.fault == 11:                # the side that is not the newest
                a, on_device = (self.h if on_device else self.d), not on_device
            if self.fault == 12:
                return self._flipping(getattr(Reader(a, on_device), name))
        return getattr(Reader(a, on_device), name)

    def _flipping(self, call):
        def run(*args, **kw):
            self.device_is_newer = not self.device_is_newer
            return call(*args, **kw)
        return run

    # -- CPU steps ---------------------------------------------------------------------------------------------------------
    def _cpu_begin(self):
        if self.fault != 1:
            self._pull()

    def _cpu_end(self):
        if self.fault != 2:
            self.host_is_newer = True

    def update_cpu(self, dt, n):
        self._cpu_begin()
        for _ in range(n):
            self.h = euler(self.h, dt, False)
        self._cpu_end()
        if self.fault != 7:
            self.cpu_acc_current = False

    def update_cpu_leapfrog(self, dt, n):
        if n == 0:
            return
        self._cpu_begin()
        if not self.cpu_acc_current:
            self.h = euler(self.h, 0.0, False)
        for _ in range(n):
            self.h = leapfrog_step(self.h, dt, False)
        self._cpu_end()
        self.cpu_acc_current = True

    def update_cpu_adaptive(self, n, eta, dt_max, span=float("inf"), prime=False, leapfrog=False):
        if n > 0:
            self._cpu_begin()
        self.h, log, res = adaptive(self.h, n, eta, dt_max, span, prime, leapfrog, self.cpu_acc_current, False)
        if n > 0:
            self._cpu_end()
            self.cpu_acc_current = leapfrog
        return log, res

    # -- GPU steps ---------------------------------------------------------------------------------------------------------
    def _gpu_begin(self, n):
        if n == 0:
            if self.fault == 8:
                self.device_is_newer = True
            return False
        if self.host_is_newer:
            if self.fault != 3 or not self.pushed:
                self.d = self.h.copy()
            self.host_is_newer, self.gpu_acc_current, self.pushed = False, False, True
        self.device_is_newer = True
        return True

    def update_gpu(self, dt, n):
        if self._gpu_begin(n):
            for _ in range(n):
                self.d = euler(self.d, dt, True)
            self.gpu_acc_current = False

    def update_gpu_leapfrog(self, dt, n):
        if self._gpu_begin(n):
            if not self.gpu_acc_current:
                self.d = euler(self.d, 0.0, True)
            for _ in range(n):
                self.d = leapfrog_step(self.d, dt, True)
            self.gpu_acc_current = True

    def update_gpu_adaptive(self, n, eta, dt_max, span=float("inf"), prime=False, leapfrog=False, stop_at_span=False):
        if not self._gpu_begin(n):
            return np.zeros(0, F32), dict(elapsed=0.0, steps=0, idle_steps=0, dt_last=0.0, dt_smallest=0.0)
        self.d, log, res = adaptive(self.d, n, eta, dt_max, span, prime, leapfrog, self.gpu_acc_current, True, stop_at_span)
        self.gpu_acc_current = leapfrog
        return log, res

    def advance_gpu(self, span, eta, dt_max, prime=False, leapfrog=False, max_steps=4096):
        return self.update_gpu_adaptive(max_steps, eta, dt_max, span, prime, leapfrog, stop_at_span=True)


class BatchReader:
    def __init__(self, members, device, ragged):
        self.readers, self.ragged = [Reader(a, device) for a in members], ragged

    def close(self):
        pass

    def _all(self, name, *args, **kw):
        """one call per member; an argument given per member -- points (B, k, 2), a list of views, centres (B, 2) -- is dealt out"""
        def of(b, x):
            if isinstance(x, list):
                return x[b]
            return x[b] if isinstance(x, np.ndarray) and x.ndim == (3 if name.endswith("_at") else 2) and name != "pair_counts" else x
        out = [getattr(r, name)(*(of(b, x) for x in args), **kw) for b, r in enumerate(self.readers)]
        return out if self.ragged or name == "energy" or isinstance(out[0], tuple) else np.stack(out)

    def __getattr__(self, name):
        if name == "fit_views":
            return lambda w, h: self._all("fit_view", w, h)
        if name not in READS:
            raise AttributeError(name)
        return lambda *args, **kw: self._all(name, *args, **kw)


class FakeWorldBatch:
    """world_batch.c in numpy: member arrays, a device copy, uploaded / device_is_newer; members may differ in size."""

    def __init__(self, particles, fault=0, ragged=False):
        self.h, self.fault, self.ragged = [np.array(p, dtype=F32) for p in particles], fault, ragged
        self.d = [np.zeros_like(p) for p in self.h]
        self.uploaded, self.device_is_newer, self.gpu_acc_current = False, False, False

    def close(self):
        pass

    def _refresh(self):
        if self.device_is_newer:
            self.h, self.device_is_newer = [p.copy() for p in self.d], False

    def member(self, b):
        if self.fault != 10:
            self._refresh()
        return self.h[b].copy()

    def particles(self):
        self._refresh()
        return [p.copy() for p in self.h] if self.ragged else np.stack(self.h)

    def __getattr__(self, name):
        if name not in READS + ("fit_views",):
            raise AttributeError(name)
        on_device = self.device_is_newer
        if name in sd.NEW_READS and self.fault == 11:          # the side that is not the newest
            on_device = not on_device
        call = getattr(BatchReader(self.d if on_device else self.h, on_device, self.ragged), name)
        if name in sd.NEW_READS and self.fault == 12:
            return FakeWorld._flipping(self, call)
        return call

    def _dts(self, dt):
        return [float(dt)] * len(self.h) if np.ndim(dt) == 0 else [float(x) for x in dt]

    def _push_once(self):
        if not self.uploaded:
            self.d, self.uploaded = [p.copy() for p in self.h], True

    def _begin(self, n):
        if n == 0:
            if self.fault == 8:
                self.device_is_newer = True
            return False
        self._push_once()
        self.device_is_newer = True
        return True

    def update_gpu(self, dt, n):
        if self._begin(n):
            for _ in range(n):
                self.d = [euler(p, d, True) for p, d in zip(self.d, self._dts(dt))]
            self.gpu_acc_current = False

    def update_gpu_leapfrog(self, dt, n):
        if self._begin(n):
            if not self.gpu_acc_current:
                self.d = [euler(p, 0.0, True) for p in self.d]
            for _ in range(n):
                self.d = [leapfrog_step(p, d, True) for p, d in zip(self.d, self._dts(dt))]
            self.gpu_acc_current = True

    def update_gpu_adaptive(self, n, eta, dt_max, span=float("inf"), prime=False, leapfrog=False, stop_at_span=False):
        if not self._begin(n):
            return np.zeros((0, len(self.h)), F32), [dict(elapsed=0.0, steps=0, idle_steps=0, dt_last=0.0, dt_smallest=0.0)] * len(self.h)
        outs = [adaptive(p, n, eta, dt_max, span, prime, leapfrog, self.gpu_acc_current, True, stop_at_span) for p in self.d]
        self.d, self.gpu_acc_current = [o[0] for o in outs], leapfrog
        made = max(len(o[1]) for o in outs)
        return np.stack([np.pad(o[1], (0, made - len(o[1]))) for o in outs], axis=1), [o[2] for o in outs]

    def advance_gpu(self, span, eta, dt_max, prime=False, leapfrog=False, max_steps=4096):
        return self.update_gpu_adaptive(max_steps, eta, dt_max, span, prime, leapfrog, stop_at_span=True)

    def update_gpu_traced(self, dt, n, every):
        def row():
            return [np.frombuffer(sd.ebits(Reader(p, True).energy()), dtype=F64) for p in self.d]
        self._push_once()
        rows = [row()]
        for k in range(n):
            self.d = [euler(p, d, True) for p, d in zip(self.d, self._dts(dt))]
            if (k + 1) % every == 0:
                rows.append(row())
        if n > 0:
            self.gpu_acc_current = False
            if self.fault != 9:
                self.device_is_newer = True
        return np.array(rows)


# ---- environments ----------------------------------------------------------------------------------------------------------------

def small_world(seed, n=20, m=11):
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=F32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 50
    a[:, 2:4] = rng.standard_normal((n, 2))
    a[:, 7] = 0.5
    a[:m, 7] = 1.5 + 3 * rng.random(m)
    a[:m, 6] = 40 * a[:m, 7] ** 3
    a = euler(euler(a, 0.01, False), 0.01, False)          # two steps in: acc is not zero
    sd.assert_premise(a)
    return a


def fake_view(w, h):
    return types.SimpleNamespace(target=(0.0, 0.0), offset=(w / 2, h / 2), zoom=w / 300.0, width=w, height=h, core_mass=1000.0)


_points = np.random.default_rng(5).standard_normal((max(sd.POINT_COUNTS), 2)).astype(F32) * 60
B, RAGGED = 3, ((20, 11), (7, 7), (33, 1), (12, 0))


def fake_env(kind, fault=0):
    base = ws.base_of(kind)
    # a reads kind: the factories of the seam's stand-in (tests/test_sequence_cpu.py), at the same scale
    more = {} if kind == base else dict(edges=read_edges, centre=read_centre(members_of(kind)), radius=30.0)
    view, points = (fake_view, lambda k: _points[:k]) if kind == base else (read_view, read_points(members_of(kind)))
    if base == "world":
        return ws.Env(kind, small_world(1), lambda s: FakeWorld(s, fault), lambda s: Reader(np.array(s, dtype=F32), True), view, points, **more)
    ragged = base == "ragged"
    start = [small_world(30 + b, n, m) for b, (n, m) in enumerate(RAGGED)] if ragged else np.stack([small_world(20 + b) for b in range(B)])
    return ws.Env(kind, start, lambda s: FakeWorldBatch(s, fault, ragged), lambda s: BatchReader([np.array(p, dtype=F32) for p in s], True, ragged),
                  view, points if kind != base else None, members=len(start), **more)


def members_of(kind):
    return {"world": 0, "batch": B, "ragged": len(RAGGED)}[ws.base_of(kind)]


def caught_by(kind, seed, fault):
    try:
        ws.check(fake_env(kind, fault), ws.generate(kind, seed, members=members_of(kind)), seed)
    except sd.SequenceMismatch as e:
        return e
    return None


def first_touch(fault, ops):
    """index of the first operation the fault could change the output of"""
    def first(pred, start=0):
        return next(i for i in range(start, len(ops)) if pred(ops[i]))

    def gpu(op):
        return op[0] in ws.GPU_STEPS and ws._moves(op)

    def cpu(op):
        return op[0] in ws.CPU_STEPS and (op[0] == "update_cpu" or ws._moves(op))
    if fault in (1, 2, 4, 5):
        return first(cpu, first(gpu) + 1)
    if fault == 3:
        return first(gpu, first(cpu, first(gpu) + 1) + 1)
    if fault == 6:
        return first(lambda op: op[0] == "particles", first(lambda op: op[0] == "update_cpu_leapfrog" and ws._moves(op)) + 1)
    if fault == 7:
        return first(lambda op: op[0] == "update_cpu", first(lambda op: op[0] in ws.CPU_STEPS and op[1].get("leapfrog") or op[0] == "update_cpu_leapfrog"))
    if fault == 8:
        return first(lambda op: op[0] in ws.GPU_STEPS and not ws._moves(op))
    if fault == 9:
        return first(lambda op: op[0] == "update_gpu_traced" and ws._moves(op))
    if fault in (11, 12):
        return first(lambda op: op[0] in sd.NEW_READS)
    return first(lambda op: op[0] == "member", first(gpu) + 1)


# ---- 1. the real library, CPU operations only ------------------------------------------------------------------------------------

_real = {}


def real_env(n, frac):
    if n not in _real:
        w = nb.World(synth(n, frac_massive=frac, seed=n)[0])
        w.update_cpu(0.01, 2)
        start = w.particles()
        w.close()
        sd.assert_premise(start)

        def view(width, height):
            return nb.RenderView.make((0.0, 0.0), (width / 2, height / 2), width / 6.0e4, width, height, 2.0e4)
        points = np.random.default_rng(78).standard_normal((max(sd.POINT_COUNTS), 2)).astype(F32) * 1.0e4
        _real[n] = ws.Env("world", start, nb.World, None, view, lambda k: points[:k])
    return _real[n]


@pytest.mark.parametrize("seed", ws.SEEDS["world"])
@pytest.mark.parametrize("row", ["chain-200", "lanes-600"])
def test_a_long_lived_world_on_the_host_cores_is_a_chain_of_fresh_ones(row, seed):
    ops = ws.cpu_only(ws.generate("world", seed))
    assert len(ops) >= ws.LENGTH // 2 and {"update_cpu", "update_cpu_leapfrog", "update_cpu_adaptive", "particles"} <= {n for n, _ in ops}
    assert ws.check(real_env(*ws.WORLD_ROWS[row]), ops, seed) > len(ops) // 2


def real_reads_env(n, frac):
    """the same start state under "world-reads", with the arguments of tests/reads_common.py held to have something to say"""
    if ("reads", n) not in _real:
        env = real_env(n, frac)
        reads_common.assert_the_reads_have_something_to_say([(env.start, int(np.count_nonzero(env.start[:, 6] > 0)))])
        f = reads_common.factories(0, env.view)
        _real[("reads", n)] = ws.Env("world-reads", env.start, nb.World, None, f["view"], f["points"], edges=f["edges"], centre=f["centre"],
                                     radius=f["radius"])
    return _real[("reads", n)]


@pytest.mark.parametrize("seed", ws.SEEDS["world-reads"])
@pytest.mark.parametrize("row", ["chain-200", "lanes-600"])
def test_a_long_lived_world_on_the_host_cores_answers_every_read_only_call_like_a_fresh_one(row, seed):
    """the host paths of tidal_at, tidal_map, profile, pair_counts and neighbours of the real library, in long sequences among
    CPU steps of every kind"""
    ops = ws.cpu_only(ws.generate("world-reads", seed))
    assert set(sd.NEW_READS) <= {n for n, _ in ops} and {"update_cpu", "update_cpu_leapfrog", "update_cpu_adaptive"} <= {n for n, _ in ops}
    assert ws.check(real_reads_env(*ws.WORLD_ROWS[row]), ops, seed) > len(ops) // 2


def test_the_host_sequences_open_no_device():
    code = ("import os, test_world_sequence_cpu as t, world_sequence as ws\n"
            "for row in ('chain-200', 'lanes-600'):\n"
            "    for seed in ws.SEEDS['world']:\n"
            "        ws.check(t.real_env(*ws.WORLD_ROWS[row]), ws.cpu_only(ws.generate('world', seed)), seed)\n"
            "    for seed in ws.SEEDS['world-reads']:\n"
            "        ws.check(t.real_reads_env(*ws.WORLD_ROWS[row]), ws.cpu_only(ws.generate('world-reads', seed)), seed)\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK')\n")
    r = child(code)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout, r.stderr)


# ---- 2. teeth ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(FAULTS_OF))
def test_without_a_fault_every_committed_seed_passes(kind):
    for seed in ws.SEEDS[kind]:
        assert caught_by(kind, seed, 0) is None


@pytest.mark.parametrize("kind,fault", [(k, f) for k in sorted(FAULTS_OF) for f in FAULTS_OF[k]])
def test_every_planted_fault_is_caught_by_a_committed_seed(kind, fault):
    caught = []
    for seed in ws.SEEDS[kind]:
        e = caught_by(kind, seed, fault)
        if e is not None:
            ops = ws.generate(kind, seed, members=members_of(kind))
            assert e.seed == seed and e.index >= first_touch(fault, ops), (FAULTS[fault], e.index, first_touch(fault, ops))
            assert e.name == (ops[e.index][0] if e.index < len(ops) else "final state")
            assert f"seed {seed}" in str(e) and sd.show(ops[0]) in str(e)
            caught.append(seed)
    assert caught, f"no committed seed of {kind} notices: {FAULTS[fault]}"


def test_a_path_error_and_stale_state_are_told_apart():
    """fault 4 answers with the right state on the wrong path, fault 5 with the device's older state"""
    seen = {}
    for fault in (4, 5):
        for seed in ws.SEEDS["world"]:
            e = caught_by("world", seed, fault)
            if e is not None and e.name in ws.PATH_READS:
                seen.setdefault(fault, str(e))
    assert "PATH ERROR" in seen[4] and "STALE STATE" not in seen[4]
    assert "STALE STATE" in seen[5] and "PATH ERROR" not in seen[5]


@pytest.mark.parametrize("kind", sorted(FAULTS_OF))
def test_the_seeds_are_the_first_pair_that_catches_every_fault(kind):
    catches = {}
    for seed in range(max(ws.SEEDS[kind]) + 1):
        try:
            if caught_by(kind, seed, 0) is None:
                catches[seed] = {f for f in FAULTS_OF[kind] if caught_by(kind, seed, f) is not None}
        except AssertionError:
            continue          # assert_covers: this seed names no sequence

    def good(pair):
        if catches[pair[0]] | catches[pair[1]] != set(FAULTS_OF[kind]):
            return False
        try:
            for members in ws.MEMBERS[kind]:
                ws.assert_union_covers(kind, [ws.generate(kind, seed, members=members) for seed in pair])
        except AssertionError:
            return False
        return True
    pairs = (p for p in itertools.combinations(sorted(catches), 2) if good(p))
    assert next(pairs) == tuple(ws.SEEDS[kind]), {s: sorted(c) for s, c in catches.items()}


@pytest.mark.parametrize("kind,members", [(k, m) for k in sorted(ws.MEMBERS) for m in ws.MEMBERS[k]])
def test_the_committed_sequences_issue_every_operation_between_them(kind, members):
    """every name of WEIGHTS[kind]; for a World and a WorldBatch every form of the adaptive calls with n > 0; for a World the
    zero-step form of every update call -- in the lists the GPU rows run"""
    lists = [ws.generate(kind, seed, members=members) for seed in ws.SEEDS[kind]]
    ws.assert_union_covers(kind, lists)
    with pytest.raises(AssertionError, match="never issue"):
        ws.assert_union_covers(kind, [[op for op in lst if op[0] != "potential"] for lst in lists])


@pytest.mark.parametrize("kind", sorted(FAULTS_OF))
def test_committed_sequences_hold_what_they_must(kind):
    for seed in ws.SEEDS[kind]:
        ops = ws.generate(kind, seed, members=members_of(kind))
        ws.assert_covers(kind, ops)
        assert len(ops) == (ws.READS_LENGTH if kind in ws.READS_BASE else ws.LENGTH) and ops == ws.generate(kind, seed, members=members_of(kind))
        if ws.base_of(kind) == "ragged":
            assert {name for name, _ in ops} <= ws.ragged_allowed(kind)
            assert not {name for name, _ in ops} & {"bounds", "fit_views", "render", "render_counts", "update_gpu_adaptive", "advance_gpu"}
        if ws.base_of(kind) == "world":
            assert not set(n for n, _ in ws.cpu_only(ops)) & set(ws.GPU_STEPS)


def test_the_generator_notices_a_dropped_reads_piece():
    ops = ws.generate("world-reads", ws.SEEDS["world-reads"][0])
    names = [n for n, _ in ops]

    def without(drop):
        return [op for i, op in enumerate(ops) if not drop(i)]
    with pytest.raises(AssertionError, match=r"neighbours\(None\)"):
        ws.assert_covers("world-reads", without(lambda i: 0 < i < len(ops) - 1 and names[i - 1] == names[i] == "neighbours" and
                                                names[i + 1] == "pair_counts"))
    with pytest.raises(AssertionError, match="particles"):
        ws.assert_covers("world-reads", without(lambda i: 0 < i < len(ops) - 1 and names[i] == "particles" and names[i - 1] in ws.EXACT_READS and
                                                names[i + 1] in ("tidal_at", "tidal_map")))
    with pytest.raises(AssertionError, match="after CPU steps"):
        ws.assert_covers("world-reads", without(lambda i: 0 < i and names[i] in ("tidal_at", "tidal_map") and names[i - 1] in ws.CPU_STEPS))
    ragged = ws.generate("ragged-reads", ws.SEEDS["ragged-reads"][0], members=len(RAGGED))
    with pytest.raises(AssertionError):
        ws.assert_covers("ragged-reads", ragged + [("bounds", {})])


def test_the_generator_notices_a_dropped_piece():
    ops = ws.generate("world", ws.SEEDS["world"][0])
    with pytest.raises(AssertionError, match="advance_gpu"):
        ws.assert_covers("world", [op for op in ops if op[0] != "advance_gpu"])
    with pytest.raises(AssertionError, match="before any push"):
        ws.assert_covers("world", ops[1:])
    with pytest.raises(AssertionError, match="leapfrog"):
        ws.assert_covers("world", [op for op in ops if op[0] != "update_gpu_leapfrog"])
    ops = ws.generate("batch", ws.SEEDS["batch"][0], members=B)
    with pytest.raises(AssertionError, match="traced"):
        ws.assert_covers("batch", [op for op in ops if op[0] != "update_gpu_traced"])
    with pytest.raises(AssertionError):
        ws.assert_covers("ragged", ops)
