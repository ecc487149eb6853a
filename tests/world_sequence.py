"""World sequence driver (TEST INFRASTRUCTURE): a long-lived World or WorldBatch against a chain of fresh ones.

The layer above the seam (world.c, world_batch.c) keeps its own state between calls: `host_is_newer`, `device_is_newer` and
`cpu_acc_current` on a World, `uploaded` and `device_is_newer` on a WorldBatch.  They decide when the array crosses between
host and device, whether a leapfrog call primes, and on which side a diagnostic runs.  The oracle is that of
tests/sequence_driver.py, one layer up:

  observed run   ONE World / WorldBatch takes the whole seeded sequence; the array is read back only where the sequence says
                 particles (or member)
  reference run  every state-moving operation gets a NEW World(state) / WorldBatch(state), the SAME call, particles().  The
                 mass partition of a partitioned array is the identity, so a fresh object holds the state in the same order
                 (asserted on the first state of every environment)
  verdict        every output and the final array equal BIT FOR BIT; no tolerance anywhere

Diagnostics and the path rule.  The host and the device paths of energy, potential and the four field calls do not agree
in bits, so the driver carries the documented rule as a one-bit model and knows both values:

  World       include/nbody_diag.h, world.c: the device answers once a GPU call (of n > 0 steps) has uploaded the array and no
              CPU update has changed it since; reading it back with particles() does not change that.  UpdateWorld_CPU marks
              the array changed for every n, n = 0 included (world.c follows the reference there); the leapfrog and adaptive
              CPU calls do nothing at all for n = 0.
  WorldBatch  include/nbody_batch_diag.h: the device answers exactly when it has stepped since the array was last read back
              (particles / member).
  device value   that of a fresh SimPipeline / SimBatch handed the state, with the same sizes and no knobs (env.device)
  host value     that of a fresh World / WorldBatch that has never stepped on the GPU

A value that equals the OTHER path's is reported as a path error, one that equals neither as stale state.  bounds,
fit_view(s), render_counts, render and timestep are bitwise the same on both paths by contract and are compared with the
fresh World directly.

The reads kinds ("world-reads", "batch-reads", "ragged-reads") add tidal_at, tidal_map, profile, pair_counts and neighbours with
the drawn arguments of sequence_driver's reads kinds (an ensemble kind: the four Phi / g field calls too).  The path rule follows
the headers: the host path of tidal_at / tidal_map runs in float64 and does not agree with the device in bits, so they join
PATH_READS and the one-bit model; profile, pair_counts and neighbours promise "bit for bit on device, host and numpy", so they are
compared with the fresh World directly and, where env.device exists, with the seam object as well (EXACT_READS).

A long-lived object that rightly skips a leapfrog call's priming launch is compared with fresh ones that make it, so these
sequences rest on the premise of sequence_driver's leapfrog kinds: start states are finite and hold no -0.0 position or
velocity (sequence_driver.assert_premise, called where the environments are built).

This module imports no GPU code: `env.make(state)` builds the object, `env.device(state)` the seam object that gives the
device values (None where no operation may reach a device), so tests/test_world_sequence_cpu.py drives the real libnbody.so
through its CPU operations, and a numpy stand-in with planted faults through all of them, with the very same code."""
import struct

import numpy as np

from sequence_driver import (ADAPT_SPAN, AT_CALLS, DT_MAX, ETA, MAP_CALLS, MAP_SIZES, MASKS, NEW_READS, POINT_COUNTS, RENDER_SIZES, SOFT,
                             STEP_DTS, TRACE_EVERY, SequenceMismatch, _make_read, _pick, _probes, _read, _views, adaptive_bits, blob,
                             ebits, show)

STEP_COUNTS = (0, 1, 2, 3, 5)          # 0: the zero-step forms, which must change nothing
ADAPT_COUNTS = (0, 1, 3, 6)
ADVANCE_MAX = 48                       # max_steps of an advance call: more than ADAPT_SPAN needs at these sizes
LENGTH = 64                            # the planted pieces are 29 operations of a World sequence: room for every drawn call
READS_LENGTH = 88                      # the reads kinds: the base kind's pieces, those of _planted_reads, and as many drawn calls
# the committed seeds: tests/test_gpu_world_sequences.py runs exactly these, tests/test_world_sequence_cpu.py says how they
# were chosen and shows that each pair catches every planted fault of its stand-in
SEEDS = {"world": (0, 1), "batch": (0, 3), "ragged": (0, 1), "world-reads": (2, 5), "batch-reads": (0, 6), "ragged-reads": (0, 1)}
# a reads kind draws everything its base kind draws, and tidal_at, tidal_map, profile, pair_counts and neighbours (an ensemble
# kind: the four Phi / g field calls too, which "batch" and "ragged" never draw), with the drawn arguments of sequence_driver's
# reads kinds.  env.view, env.points, env.edges, env.centre and env.radius are those of sequence_driver.Env
READS_BASE = {"world-reads": "world", "batch-reads": "batch", "ragged-reads": "ragged"}
# the member counts the rows run with: what a sequence draws for member() depends on them
MEMBERS = {"world": (0,), "batch": (5, 3), "ragged": (12,), "world-reads": (0,), "batch-reads": (5, 3), "ragged-reads": (12,)}


def base_of(kind):
    return READS_BASE.get(kind, kind)

# the chain, lane-split and classic routes with the frac_massive of sequence_driver.PIPE_ROWS; the ensembles of its GPU rows
WORLD_ROWS = {"chain-200": (200, 0.5), "lanes-600": (600, 0.5), "classic-4133": (4133, 1.0)}
BATCH_ROWS = {"chain-5x250": (5, 250), "lanes-3x800": (3, 800)}

CPU_STEPS = ("update_cpu", "update_cpu_leapfrog", "update_cpu_adaptive")
GPU_STEPS = ("update_gpu", "update_gpu_leapfrog", "update_gpu_adaptive", "advance_gpu", "update_gpu_traced")
STEPS = CPU_STEPS + GPU_STEPS
READ_BACK = ("particles", "member")
# the host path of the tidal calls runs in float64 and does not agree with the device in bits (include/nbody_tidal.h,
# nbody_batch_tidal.h): the path rule and its one-bit model hold for them as for the other field calls
PATH_READS = ("energy", "potential", "potential_at", "acceleration_at", "potential_map", "acceleration_map", "tidal_at", "tidal_map")
# "bit for bit on device, host and numpy" (include/nbody_profile.h, nbody_paircount.h, nbody_neighbour.h): compared with the
# fresh World directly and, where env.device exists, with the seam object as well
EXACT_READS = ("profile", "pair_counts", "neighbours")
BITWISE_READS = ("timestep", "bounds", "fit_view", "fit_views", "render_counts", "render") + EXACT_READS
# every operation of the World kind that cannot reach a device: what the CPU-only run keeps
CPU_ONLY = CPU_STEPS + READ_BACK + PATH_READS + BITWISE_READS

WEIGHTS = {
    "world": ({"update_cpu": 0.05, "update_gpu": 0.05, "update_cpu_leapfrog": 0.03, "update_gpu_leapfrog": 0.04,
               "update_cpu_adaptive": 0.03, "update_gpu_adaptive": 0.03, "advance_gpu": 0.02},
              {"timestep": 0.06, "particles": 0.07, "energy": 0.08, "potential": 0.07, "potential_at": 0.05, "acceleration_at": 0.05,
               "potential_map": 0.05, "acceleration_map": 0.05, "bounds": 0.04, "fit_view": 0.04, "render_counts": 0.05, "render": 0.06}),
    "batch": ({"update_gpu": 0.10, "update_gpu_leapfrog": 0.08, "update_gpu_adaptive": 0.05, "advance_gpu": 0.03, "update_gpu_traced": 0.07},
              {"particles": 0.08, "member": 0.08, "energy": 0.12, "potential": 0.11, "bounds": 0.06, "fit_views": 0.05,
               "render_counts": 0.08, "render": 0.09}),
    # include/nbody_batch_ragged.h lists these, and the field, tidal, profile, pair-count and neighbour calls that "ragged-reads"
    # draws; the bounds, fit and render calls abort on a ragged batch, and it has no adaptive or leapfrog steps
    "ragged": ({"update_gpu": 0.20, "update_gpu_traced": 0.13},
               {"particles": 0.14, "member": 0.14, "energy": 0.20, "potential": 0.19}),
    # the reads kinds: the steps of the base kind; the new calls take about a third of the whole from the other calls
    "world-reads": ({"update_cpu": 0.05, "update_gpu": 0.05, "update_cpu_leapfrog": 0.03, "update_gpu_leapfrog": 0.04,
                     "update_cpu_adaptive": 0.03, "update_gpu_adaptive": 0.03, "advance_gpu": 0.02},
                    {"timestep": 0.03, "particles": 0.05, "energy": 0.04, "potential": 0.04, "potential_at": 0.03, "acceleration_at": 0.03,
                     "potential_map": 0.03, "acceleration_map": 0.03, "bounds": 0.02, "fit_view": 0.02, "render_counts": 0.03, "render": 0.03,
                     "tidal_at": 0.06, "tidal_map": 0.06, "profile": 0.07, "pair_counts": 0.07, "neighbours": 0.09}),
    "batch-reads": ({"update_gpu": 0.10, "update_gpu_leapfrog": 0.08, "update_gpu_adaptive": 0.05, "advance_gpu": 0.03, "update_gpu_traced": 0.07},
                    {"particles": 0.06, "member": 0.06, "energy": 0.05, "potential": 0.05, "bounds": 0.03, "fit_views": 0.03,
                     "render_counts": 0.04, "render": 0.04, "potential_at": 0.03, "acceleration_at": 0.03, "potential_map": 0.03,
                     "acceleration_map": 0.03, "tidal_at": 0.04, "tidal_map": 0.04, "profile": 0.05, "pair_counts": 0.05, "neighbours": 0.06}),
    "ragged-reads": ({"update_gpu": 0.20, "update_gpu_traced": 0.13},
                     {"particles": 0.08, "member": 0.08, "energy": 0.07, "potential": 0.07, "potential_at": 0.03, "acceleration_at": 0.03,
                      "potential_map": 0.03, "acceleration_map": 0.03, "tidal_at": 0.04, "tidal_map": 0.04, "profile": 0.06,
                      "pair_counts": 0.06, "neighbours": 0.08}),
}
RAGGED_ALLOWED = frozenset(WEIGHTS["ragged"][0]) | frozenset(WEIGHTS["ragged"][1])
RAGGED_READS_ALLOWED = frozenset(WEIGHTS["ragged-reads"][0]) | frozenset(WEIGHTS["ragged-reads"][1])


def ragged_allowed(kind):
    return RAGGED_READS_ALLOWED if kind == "ragged-reads" else RAGGED_ALLOWED


class Env:
    """kind; the first state; make(state) -> World / WorldBatch; device(state) -> the seam object with that state (or None: no
    operation of the sequence may reach a device); view(w, h); points(k); members (0: a single World)."""

    def __init__(self, kind, start, make, device, view, points, members=0, edges=None, centre=None, radius=None):
        self.kind, self.start, self.make, self.device, self.view, self.points, self.members = kind, start, make, device, view, points, members
        self.edges, self.centre, self.radius = edges, centre, radius          # a reads kind: as in sequence_driver.Env


# ---- one operation -------------------------------------------------------------------------------------------------------------

def raw(x):
    """a RenderView (or a list of them), an array -> bytes"""
    if isinstance(x, (list, tuple)):
        return b"".join(raw(v) for v in x)
    return blob(x) if isinstance(x, np.ndarray) else bytes(x)


def _dt(a, env):
    if not a.get("per_member"):
        return a["dt"]
    return [a["dt"] * (1.0 + 0.1 * b) for b in range(env.members)]


def _adaptive_kw(a):
    return {k: a[k] for k in ("span", "prime", "leapfrog") if a.get(k)}


def apply(obj, op, env):
    """Issue one operation on a World / WorldBatch (or, for the PATH_READS, on the seam object of env.device); bytes or None."""
    name, a = op
    if base_of(env.kind) == "ragged":
        assert name in ragged_allowed(env.kind), f"{name}: include/nbody_batch_ragged.h does not list it; the generator must never emit it"
    if name in ("update_cpu", "update_gpu", "update_cpu_leapfrog", "update_gpu_leapfrog"):
        getattr(obj, name)(_dt(a, env), a["n"])
    elif name in ("update_cpu_adaptive", "update_gpu_adaptive"):
        return adaptive_bits(getattr(obj, name)(a["n"], ETA, DT_MAX, **_adaptive_kw(a)))
    elif name == "advance_gpu":
        return adaptive_bits(obj.advance_gpu(a["span"], ETA, DT_MAX, max_steps=ADVANCE_MAX, **_adaptive_kw(dict(a, span=None))))
    elif name == "update_gpu_traced":
        return blob(obj.update_gpu_traced(_dt(a, env), a["n"], a["every"]))
    elif name == "particles":
        return blob(obj.particles())
    elif name == "member":
        return blob(obj.member(a["b"]))
    elif name == "timestep":
        return struct.pack("<d", obj.timestep(ETA, DT_MAX))
    elif name == "energy":
        return ebits(obj.energy())
    elif name == "potential":
        return blob(obj.potential())
    elif name == "potential_at":
        return blob(obj.potential_at(_probes(a, env), SOFT))
    elif name == "acceleration_at":
        return blob(obj.acceleration_at(_probes(a, env), SOFT))
    elif name == "potential_map":
        return blob(obj.potential_map(_views(a, env), SOFT))
    elif name == "acceleration_map":
        return blob(obj.acceleration_map(_views(a, env), SOFT))
    elif name in NEW_READS:
        return blob(_read(obj, name, a, env))
    elif name == "bounds":
        return blob(obj.bounds())
    elif name in ("fit_view", "fit_views"):
        return raw(getattr(obj, name)(a["w"], a["h"]))
    elif name in ("render_counts", "render"):
        return blob(getattr(obj, name)(env.view(a["w"], a["h"])))
    else:
        raise ValueError(f"unknown operation {name}")
    return None


# ---- the path model ------------------------------------------------------------------------------------------------------------

def device_answers(kind, on_device, op):
    """The one-bit model after `op` (module docstring): does the device answer the next diagnostic?"""
    name, a = op
    if name in GPU_STEPS:
        return True if (name == "advance_gpu" or a["n"] > 0) else on_device
    if base_of(kind) == "world":
        if name == "update_cpu" or (name in CPU_STEPS and a["n"] > 0):
            return False
    elif name in READ_BACK:
        return False
    return on_device


# ---- the run -------------------------------------------------------------------------------------------------------------------

def _fresh(env, state, op):
    """(output, state after) of the operation on a new object holding `state`"""
    obj = env.make(state)
    out = apply(obj, op, env)
    after = obj.particles() if op[0] in STEPS else state
    obj.close()
    return out, after


def _device_value(env, state, op):
    assert env.device is not None, f"{show(op)}: the model says the device answers, and this run may not reach one"
    seam = env.device(state)
    out = apply(seam, op, env)
    seam.close()
    return out


def _differs(got, want):
    if got is None or want is None:
        return "one of them returned nothing"
    return f"{sum(x != y for x, y in zip(got, want)) + abs(len(got) - len(want))} of {len(want)} bytes"


def check(env, ops, seed=None):
    """Raises SequenceMismatch naming the first operation whose output differs; returns the number of outputs compared."""
    first = env.make(env.start)
    assert blob(first.particles()) == blob(env.start), "the start state is not partitioned: a fresh object would reorder it"
    first.close()
    obj, state, on_device, compared = env.make(env.start), env.start, False, 0
    for i, op in enumerate(ops):
        name = op[0]
        got = apply(obj, op, env)
        if name in PATH_READS:
            host = _fresh(env, state, op)[0]
            want = _device_value(env, state, op) if on_device else host
            if got != want:
                other = host if on_device else (_device_value(env, state, op) if env.device is not None else None)
                side = ("device", "host") if on_device else ("host", "device")
                what = (f"PATH ERROR: the rule says the {side[0]} answers, the value is the {side[1]} path's" if got == other else
                        f"STALE STATE: the {side[0]} should answer; the value is that of neither path for this state, {_differs(got, want)}")
                raise SequenceMismatch(seed, i, name, ops, what)
        elif name in READ_BACK:
            want = blob(state[op[1]["b"]]) if name == "member" else blob(state)
            if got != want:
                raise SequenceMismatch(seed, i, name, ops, "the array read back, " + _differs(got, want))
        else:
            want, state = _fresh(env, state, op)
            if got != want:
                raise SequenceMismatch(seed, i, name, ops, _differs(got, want))
            if name in EXACT_READS and env.device is not None:
                seam = _device_value(env, state, op)
                if got != seam:
                    raise SequenceMismatch(seed, i, name, ops, "the seam object's value for this state, " + _differs(got, seam))
        compared += got is not None
        on_device = device_answers(env.kind, on_device, op)
    final = blob(obj.particles())
    obj.close()
    if final != blob(state):
        raise SequenceMismatch(seed, len(ops), "final state", ops, "particles() after the last operation")
    return compared + 1


# ---- the generator -------------------------------------------------------------------------------------------------------------

def _make(rng, kind, name, members):
    if kind in READS_BASE:
        if name in AT_CALLS + MAP_CALLS + NEW_READS:
            return _make_read(rng, name, kind != "world-reads")
        kind = READS_BASE[kind]
    if name in ("update_cpu", "update_gpu", "update_cpu_leapfrog", "update_gpu_leapfrog", "update_gpu_traced"):
        a = {"n": int(_pick(rng, STEP_COUNTS)), "dt": float(_pick(rng, STEP_DTS))}
        if kind != "world":
            a["per_member"] = bool(rng.random() < 0.5)
        if name == "update_gpu_traced":
            a["every"] = int(_pick(rng, TRACE_EVERY))
        return name, a
    if name in ("update_cpu_adaptive", "update_gpu_adaptive", "advance_gpu"):
        a = {"span": ADAPT_SPAN} if name == "advance_gpu" else {"n": int(_pick(rng, ADAPT_COUNTS))}
        if name != "advance_gpu" and rng.random() < 0.25:
            a["span"] = ADAPT_SPAN
        if rng.random() < 0.3:
            a["prime"] = True
        if rng.random() < 0.4:
            a["leapfrog"] = True
        return name, a
    if name in ("potential_at", "acceleration_at"):
        return name, {"count": int(_pick(rng, POINT_COUNTS))}
    if name in ("potential_map", "acceleration_map"):
        w, h = _pick(rng, MAP_SIZES)
        return name, {"w": w, "h": h}
    if name in ("render_counts", "render", "fit_view", "fit_views"):
        w, h = _pick(rng, RENDER_SIZES)
        return name, {"w": w, "h": h}
    if name == "member":
        return name, {"b": int(rng.integers(members))}
    return name, {}


def _steps(rng, kind, name, members, leapfrog=None):
    """a drawn stepping operation that does step (n > 0)"""
    op = _make(rng, kind, name, members)
    if "n" in op[1]:
        op[1]["n"] = max(op[1]["n"], 1 + int(rng.integers(3)))
    if leapfrog is not None:
        op[1].pop("prime", None)
        op[1].pop("leapfrog", None)
        if leapfrog:
            op[1]["leapfrog"] = True
    return op


def _planted(rng, kind, members):
    """The pieces every sequence holds, in this order (assert_covers finds each on the list itself)."""
    def s(name, **kw):
        return _steps(rng, kind, name, members, **kw)
    diag = _make(rng, kind, _pick(rng, ("energy", "potential")), members)
    again = _make(rng, kind, _pick(rng, ("energy", "potential")), members)
    base = base_of(kind)
    if base == "world":
        def adaptive(name, flag):
            op = s(name, leapfrog=flag == "leapfrog")
            if flag == "prime":
                op[1]["prime"] = True
            return op

        def zero(name):
            op = _make(rng, kind, name, members)
            op[1]["n"] = 0
            return op
        return [
            # an n = 0 GPU call before any push, then a diagnostic: the host answers
            [("update_gpu", {"n": 0, "dt": 0.01}), diag],
            # a CPU step directly after GPU steps pulls first; GPU steps directly after a CPU step push; then, the device
            # newer, a plain adaptive CPU call: its first criterion is answered from the device, and the step pulls
            [s("update_gpu"), s("update_cpu"), s("update_gpu"), s("update_cpu_adaptive", leapfrog=False)],
            # an advance between two fixed GPU updates; a diagnostic after GPU steps, particles(), the same diagnostic: a
            # read-back does not move the path
            [s("update_gpu"), _make(rng, kind, "advance_gpu", members), s("update_gpu"), again, ("particles", {}), again],
            # an Euler CPU update between two CPU leapfrog calls, and every change of side: each primes again
            [s("update_cpu_leapfrog"), s("update_cpu"), s("update_cpu_leapfrog"), s("update_gpu_leapfrog"), ("particles", {}),
             s("update_cpu_leapfrog")],
            # the adaptive calls in their leapfrog and primed forms, changing sides between them
            [adaptive("update_gpu_adaptive", "leapfrog"), adaptive("update_cpu_adaptive", "leapfrog"), adaptive("update_gpu_adaptive", "prime"),
             adaptive("update_cpu_adaptive", "prime")],
            # the zero-step forms behind GPU steps change nothing, not even the side that answers -- but for UpdateWorld_CPU,
            # which marks the array changed (module docstring), so the host answers after it
            [s("update_gpu"), zero("update_cpu_leapfrog"), zero("update_cpu_adaptive"), zero("update_gpu"), zero("update_gpu_leapfrog"),
             zero("update_gpu_adaptive"), again, zero("update_cpu"), again],
        ]
    first = [("update_gpu_traced", {"n": 0, "dt": 0.01, "per_member": False, "every": 1}), diag]   # traced, n = 0, never stepped
    later = [s("update_gpu_traced"), ("update_gpu_traced", {"n": 0, "dt": 0.01, "per_member": True, "every": 2}), again, ("particles", {}), again]
    if base == "ragged":
        return [first, later, [s("update_gpu"), ("member", {"b": int(rng.integers(members))})]]
    return [[("update_gpu", {"n": 0, "dt": 0.01, "per_member": False}), diag] + first, later,
            [s("update_gpu"), _make(rng, kind, "advance_gpu", members), s("update_gpu")],
            [s("update_gpu_leapfrog"), s("update_gpu_leapfrog"), ("member", {"b": int(rng.integers(members))}), s("update_gpu_leapfrog")]]


def _segment(rng, kind, count, members):
    step_w, rest_w = WEIGHTS[kind]
    names = list(step_w) + list(rest_w)
    p = np.array([step_w[n] for n in step_w] + [rest_w[n] for n in rest_w])
    p = p / p.sum()
    return [_make(rng, kind, names[int(rng.choice(len(names), p=p))], members) for _ in range(count)]


def _planted_reads(rng, kind, members):
    """The pieces a reads kind adds (T: tidal_at or tidal_map, E: one of EXACT_READS; the same letter is the same call):
      GPU steps, neighbours(radius, A, B), neighbours(None, C, D), pair_counts, neighbours(radius, C, D)   (A, B) != (C, D)
                                    on the device: the long-lived object's one scratch, in which the counts of the first call
                                    lie where the last one adds and the pair-count table lies over the keys
      GPU steps, T, E, particles, T, E
                                    the device answers both; a read-back leaves the path of a World where it is and moves
                                    that of a WorldBatch to the host; E is the same in bits on either side
      a World: CPU steps, T, E      the host answers, in float64 for T, and E is still the same in bits"""
    base = READS_BASE[kind]

    def gpu():
        return _steps(rng, kind, "update_gpu", members)
    first = (_pick(rng, MASKS), _pick(rng, MASKS))
    second = first
    while second == first:
        second = (_pick(rng, MASKS), _pick(rng, MASKS))

    def neigh(radius, masks):
        return "neighbours", {"radius": radius, "receivers": masks[0], "sources": masks[1]}
    t, e = _make(rng, kind, _pick(rng, ("tidal_at", "tidal_map")), members), _make(rng, kind, _pick(rng, EXACT_READS), members)
    pieces = [[gpu(), neigh(True, first), neigh(False, second), _make(rng, kind, "pair_counts", members), neigh(True, second)],
              [gpu(), t, e, ("particles", {}), t, e]]
    if base == "world":
        pieces.append([_steps(rng, kind, "update_cpu", members), t, e])
    return pieces


def generate(kind, seed, length=None, members=0):
    """The sequence of (kind, seed): the planted pieces in their order, the first one first (nothing may push before it),
    drawn segments between them and behind the last.  A reads kind: a stream of its own, the base kind's pieces and then its own."""
    length = (READS_LENGTH if kind in READS_BASE else LENGTH) if length is None else length
    if kind in READS_BASE:
        rng = np.random.default_rng([seed, len(kind), sorted(READS_BASE).index(kind) + 1])
        planted = _planted(rng, kind, members) + _planted_reads(rng, kind, members)
    else:
        rng = np.random.default_rng([seed, len(kind)])
        planted = _planted(rng, kind, members)
    free = max(length - sum(len(p) for p in planted), len(planted))
    ops = []
    for i, piece in enumerate(planted):
        ops += piece + _segment(rng, kind, free // len(planted) + (1 if i < free % len(planted) else 0), members)
    assert_covers(kind, ops)
    return ops


def cpu_only(ops):
    """The World sequence restricted to the operations that cannot reach a device."""
    return [op for op in ops if op[0] in CPU_ONLY]


def _moves(op):
    return op[0] == "advance_gpu" or (op[0] in STEPS and op[1]["n"] > 0)


def _run(ops, *preds):
    """do `preds` hold for consecutive operations somewhere on the list?"""
    return any(all(f(op) for f, op in zip(preds, ops[i:])) for i in range(len(ops) - len(preds) + 1))


def assert_union_covers(kind, lists):
    """What the committed sequences of a kind must hold BETWEEN them: every operation the kind draws, and the adaptive calls
    (where the kind has them) in each drawn form, with n > 0.  The seeds are chosen so that this holds
    (tests/test_world_sequence_cpu.py)."""
    ops = [op for lst in lists for op in lst]
    every = set(WEIGHTS[kind][0]) | set(WEIGHTS[kind][1])
    assert every <= {name for name, _ in ops}, f"the committed {kind} sequences never issue {sorted(every - {name for name, _ in ops})}"
    if kind in READS_BASE:          # neighbours with and without a radius; an ensemble: each argument one for all and one per member
        for radius in (True, False):
            assert any(n == "neighbours" and a["radius"] == radius for n, a in ops), f"no neighbours with radius {radius}"
        for what, calls in (("points", AT_CALLS), ("views", MAP_CALLS), ("centres", ("profile",))) if kind != "world-reads" else ():
            for per_member in (True, False):
                assert any(n in calls and a["per_member"] == per_member for n, a in ops), f"no {what} with per_member {per_member}"
        kind = READS_BASE[kind]

    def has(name, *flags):
        return any(n == name and a.get("n", 1) > 0 and all(a.get(f) for f in flags) for n, a in ops)
    if kind != "ragged":
        for flag in ((), ("leapfrog",), ("prime",), ("span",)):
            assert has("update_gpu_adaptive", *flag), f"no update_gpu_adaptive of n > 0 with {flag or 'nothing else'}"
        assert has("advance_gpu", "leapfrog") and has("advance_gpu", "prime"), "no advance_gpu with leapfrog, or none with prime"
        assert any(n == "update_gpu_traced" and a["n"] > 0 and a.get("per_member") for n, a in ops) or kind == "world"
    if kind == "world":
        assert has("update_cpu_adaptive", "leapfrog") and has("update_cpu_adaptive", "prime"), "no update_cpu_adaptive with leapfrog, or none with prime"
        for name in CPU_STEPS + ("update_gpu", "update_gpu_leapfrog", "update_gpu_adaptive"):
            assert any(n == name and a["n"] == 0 for n, a in ops), f"no zero-step form of {name}"


def assert_covers(kind, ops):
    """What every sequence must contain, asserted on the list itself."""
    names = [name for name, _ in ops]

    def gpu(op):
        return op[0] in GPU_STEPS and _moves(op)

    def cpu(op):
        return op[0] in CPU_STEPS and _moves(op)

    def is_(name, **kw):
        return lambda op: op[0] == name and all(op[1].get(k) == v for k, v in kw.items())

    def diag(op):
        return op[0] in PATH_READS
    pushed = next((i for i, op in enumerate(ops) if gpu(op)), len(ops))
    allowed = ragged_allowed(kind)
    if kind in READS_BASE:          # the pieces of _planted_reads
        def neigh(radius):
            return lambda op: op[0] == "neighbours" and op[1]["radius"] == radius

        def masks(op):
            return op[1]["receivers"], op[1]["sources"]
        assert any(gpu(g) and neigh(True)(a) and neigh(False)(b) and c[0] == "pair_counts" and neigh(True)(d) and masks(b) == masks(d) != masks(a)
                   for g, a, b, c, d in zip(ops, ops[1:], ops[2:], ops[3:], ops[4:])), \
            "no neighbours(radius), neighbours(None) under other masks, pair_counts, neighbours(radius) under those masks behind GPU steps"
        assert any(gpu(g) and t[0] in ("tidal_at", "tidal_map") and e[0] in EXACT_READS and p[0] == "particles" and (t, e) == (t2, e2)
                   for g, t, e, p, t2, e2 in zip(ops, ops[1:], ops[2:], ops[3:], ops[4:], ops[5:])), \
            "no tidal call and exact read after GPU steps, particles(), the same two"
        if kind == "world-reads":
            assert _run(ops, cpu, lambda op: op[0] in ("tidal_at", "tidal_map"), lambda op: op[0] in EXACT_READS), \
                "no tidal call and exact read directly after CPU steps"
        kind = READS_BASE[kind]
    if kind == "ragged":
        assert set(names) <= allowed, sorted(set(names) - allowed)
    if kind == "world":
        assert _run(ops[:pushed], lambda op: op[0] in GPU_STEPS and not _moves(op), diag), "no n = 0 GPU call before any push with a diagnostic behind it"
        assert _run(ops, gpu, cpu, gpu), "no CPU step directly after GPU steps with GPU steps directly after it"
        assert any(_run(ops, gpu, is_(d), is_("particles"), is_(d)) for d in PATH_READS), "no diagnostic after GPU steps, particles(), the same diagnostic"
        lf = is_("update_cpu_leapfrog")
        assert _run(ops, lambda op: lf(op) and _moves(op), lambda op: op[0] == "update_gpu_leapfrog" and _moves(op), is_("particles"),
                    lambda op: lf(op) and _moves(op)), "no CPU leapfrog, GPU leapfrog, particles(), CPU leapfrog"
        assert _run(ops, lambda op: lf(op) and _moves(op), lambda op: is_("update_cpu")(op) and _moves(op), lambda op: lf(op) and _moves(op)), \
            "no Euler CPU update between two CPU leapfrog calls"
        assert _run(ops, gpu, lambda op: op[0] == "update_cpu_adaptive" and _moves(op) and not op[1].get("prime") and not op[1].get("leapfrog")), \
            "no plain update_cpu_adaptive while the device is newer"
        assert _run(ops, lambda op: is_("update_gpu")(op) and _moves(op), is_("advance_gpu"), lambda op: is_("update_gpu")(op) and _moves(op)), \
            "no advance_gpu between two fixed GPU updates"
    else:
        assert _run(ops[:pushed], is_("update_gpu_traced", n=0), diag), "no traced update of n = 0 on a batch that has never stepped"
        assert _run(ops[pushed:], is_("update_gpu_traced", n=0)), "no traced update of n = 0 after steps"
        assert any(_run(ops, gpu, is_("update_gpu_traced", n=0), is_(d), is_("particles"), is_(d)) for d in ("energy", "potential")), \
            "no diagnostic after GPU steps, particles(), the same diagnostic"
        assert _run(ops, lambda op: is_("update_gpu_traced")(op) and _moves(op)), "no traced update of n > 0"
        if kind == "batch":
            assert _run(ops[:pushed], is_("update_gpu", n=0), diag), "no n = 0 GPU call before any push with a diagnostic behind it"
            assert _run(ops, lambda op: is_("update_gpu")(op) and _moves(op), is_("advance_gpu"), lambda op: is_("update_gpu")(op) and _moves(op)), \
                "no advance_gpu between two fixed GPU updates"
    if kind == "world":
        assert _run(ops, lambda op: op[0] == "update_gpu_adaptive" and _moves(op) and op[1].get("leapfrog"),
                    lambda op: op[0] == "update_cpu_adaptive" and _moves(op) and op[1].get("leapfrog")), "no adaptive leapfrog call on each side in a row"
        zeros = [lambda op, name=name: op[0] == name and op[1]["n"] == 0 for name in
                 ("update_cpu_leapfrog", "update_cpu_adaptive", "update_gpu", "update_gpu_leapfrog", "update_gpu_adaptive")]
        assert _run(ops, gpu, *zeros, diag, is_("update_cpu", n=0), diag), "no run of the zero-step forms behind GPU steps with diagnostics"
    stepping = sum(_moves(op) for op in ops) / len(names)
    assert 0.2 <= stepping <= 0.5, f"{stepping:.2f} of the operations step"
