"""Sequence driver (TEST INFRASTRUCTURE): a long-lived object against a chain of fresh ones.

A SimPipeline or SimBatch carries state between calls that its caller cannot see: the position double buffer and its phase
bit, cached hipGraph chains and the device-side step size, the adaptive head, scratch buffers with their regrow paths, the
read-back bookkeeping.  The oracle here needs none of it written down: a long-lived object must be INDISTINGUISHABLE from a
chain of fresh ones.

  sequence       a seeded list of operations (name, arguments)
  observed run   ONE object takes the whole sequence; every output is recorded; the state is read back only where the
                 sequence says get_data
  reference run  every operation gets a NEW object with the same sizes and knobs: set_data(state before), the SAME call with
                 the same arguments (never a cut-up one: the launch shape may depend on the step count), get_data(), close()
  verdict        every recorded output and the final state equal BIT FOR BIT; no tolerance anywhere

set_data uploads pos, vel, acc, mass and radius, so get_data -> set_data carries the whole state, and a fresh object's result
is a function of (state, knobs, call).  The one pair of operations that belongs together is update_adaptive_async(n) ...
adaptive_collect(n): the reference collects on the fresh object that took the async call and hands that output over when the
sequence reaches adaptive_collect (only operations that make no step may stand between the two).

This module imports no GPU code: `make` builds the object and `env` (Env below) turns plain arguments into the objects the
calls want, so tests/test_sequence_cpu.py drives a numpy stand-in with planted faults through the very same code."""
import struct

import numpy as np

STEP_COUNTS = (1, 2, 3, 7, 20, 33)
STEP_DTS = (0.01, 0.005, 0.02)
ADAPT_COUNTS = (1, 3, 6)          # odd and even: an odd call leaves the other position buffer current
ETA, DT_MAX = 0.1, 1.0
ADAPT_SPAN = 0.03                 # short enough that a call of several steps ends inside it now and then
POINT_COUNTS = (1, 65, 300)       # growing: the scratch of the field calls regrows
MAP_SIZES = ((16, 9), (40, 30))
RENDER_SIZES = ((32, 18), (80, 45))
SOFT = 0.75
TRACE_EVERY = (1, 2, 5)
LENGTH = 40
# the committed seeds: tests/test_gpu_sequences.py runs exactly these, and tests/test_sequence_cpu.py shows that the
# "pipeline" ones catch every planted fault
SEEDS = {"pipeline": (5, 8, 11), "batch": (5, 8), "ragged": (5, 8)}

# name -> (N, frac_massive, configure knobs): the smallest sizes at which each step route and launch shape exists
# (tests/test_gpu_sequences.py, tests/test_gpu_adaptive.py).  At N = 9 000 the auto rule drops the finish kernel of a split
# step (N x M >= 4e7), so the row that is about the finish kernel switches the fused form off, and the other one pins it on
# the way test_fused_finish_equals_the_two_kernel_form does.
PIPE_ROWS = {
    "chain-200": (200, 0.5, {}),                                   # the one-workgroup chain in auto mode
    "lanes-600": (600, 0.5, {}),                                   # the lane-split route
    "lanes-600-graph1": (600, 0.5, dict(graph=1)),
    "classic-4133": (4133, 1.0, {}),                               # the classic route; 17 criterion workgroups, a 37-row tail
    "classic-4133-graph0": (4133, 1.0, dict(graph=0)),
    "classic-4133-graph2": (4133, 1.0, dict(graph=2)),
    "classic-4133-lds": (4133, 1.0, dict(variant=0)),
    "split3-finish-9000": (9000, 0.5, dict(split=3, fused_finish=0)),
    "fused-finish-9000": (9000, 0.5, dict(fused_finish=1, lanes=1)),
    "passes2-1500": (1500, 0.6, dict(passes=2)),
    "lanes4-w8-900": (900, 0.4, dict(lanes=4, w=8)),
}

FIXED = ("update", "step_async", "trace")
ADAPTIVE = ("update_adaptive", "update_adaptive_async")
STEPPING = FIXED + ADAPTIVE
ASYNC = ("step_async", "update_adaptive_async")
DIAGNOSTICS = ("energy", "potential", "potential_at", "acceleration_at", "potential_map", "acceleration_map", "bounds",
               "render_counts", "render")

# name -> weight; the stepping operations of a kind sum to 1/3, everything else to 2/3
WEIGHTS = {
    "pipeline": ({"update": 0.12, "step_async": 0.07, "update_adaptive": 0.08, "update_adaptive_async": 0.06},
                 {"timestep": 0.06, "energy": 0.07, "potential": 0.06, "potential_at": 0.05, "acceleration_at": 0.05,
                  "potential_map": 0.05, "acceleration_map": 0.05, "bounds": 0.04, "render_counts": 0.05, "render": 0.06,
                  "get_data": 0.05, "set_data": 0.04, "sync": 0.04}),
    "batch": ({"update": 0.12, "step_async": 0.07, "update_adaptive": 0.08, "trace": 0.06},
              {"energy": 0.11, "potential": 0.10, "bounds": 0.07, "render_counts": 0.09, "render": 0.10, "get_data": 0.07,
               "get_member": 0.07, "set_data": 0.06}),
    # include/nbody_batch_ragged.h: steps, trace, energy, potential, get, set -- NOTHING else (render, bounds and adaptive
    # calls abort on a ragged ensemble by contract)
    "ragged": ({"update": 0.15, "step_async": 0.10, "trace": 0.08},
               {"energy": 0.18, "potential": 0.17, "get_data": 0.12, "get_member": 0.10, "set_data": 0.10}),
}
RAGGED_ALLOWED = frozenset(WEIGHTS["ragged"][0]) | frozenset(WEIGHTS["ragged"][1])


class Env:
    """What a sequence runs on: the state it starts from, the state set_data brings in, the member count of an ensemble (0: a
    single world) and two factories that turn plain arguments into what the calls take."""

    def __init__(self, kind, start, other, view, points, members=0):
        self.kind, self.start, self.other, self.view, self.points, self.members = kind, start, other, view, points, members


class SequenceMismatch(AssertionError):
    def __init__(self, seed, index, name, ops, what):
        self.seed, self.index, self.name = seed, index, name
        before = "\n".join(f"    {i:3d}  {show(op)}" for i, op in enumerate(ops[:index]))
        at = show(ops[index]) if index < len(ops) else "the final state"
        super().__init__(f"seed {seed}: operation {index} [{at}] differs between the long-lived object and a fresh one ({what}).\n"
                         f"  operations before it:\n{before}")


def show(op):
    name, args = op
    return f"{name}({', '.join(f'{k}={v}' for k, v in args.items())})"


# ---- outputs as bytes ----------------------------------------------------------------------------------------------------------

def blob(x):
    """arrays, lists of arrays (a ragged ensemble), None -> bytes"""
    if x is None:
        return None
    if isinstance(x, (list, tuple)):
        return b"".join(blob(a) for a in x)
    return np.ascontiguousarray(x).tobytes()


def ebits(e):
    """one energy dict -> its eight doubles (the field order of tests/test_gpu_ragged.py ebits); a list of them -> all"""
    if isinstance(e, list):
        return b"".join(ebits(x) for x in e)
    flat = []
    for k in ("kinetic", "potential", "mass", "momentum", "angular_momentum", "center_of_mass"):
        v = e[k]
        flat += list(v) if isinstance(v, tuple) else [v]
    return struct.pack("<8d", *flat)


def rbits(res):
    """the result of an adaptive call (one dict, or one per member)"""
    if isinstance(res, list):
        return b"".join(rbits(r) for r in res)
    return struct.pack("<dIIff", res["elapsed"], res["steps"], res["idle_steps"], res["dt_last"], res["dt_smallest"])


def adaptive_bits(out):
    log, res = out
    return np.ascontiguousarray(log, dtype=np.float32).tobytes() + rbits(res)


# ---- one operation -------------------------------------------------------------------------------------------------------------

def _dt(args, env):
    """one step size for all, or one per member (the ladder of tests/test_gpu_ragged.py DTS)"""
    if not args.get("per_member"):
        return args["dt"]
    return [args["dt"] * (1.0 + 0.1 * b) for b in range(env.members)]


def _adaptive_kw(args):
    kw = {}
    if args.get("span"):
        kw["span"] = args["span"]
    if args.get("prime"):
        kw["prime"] = True
    return kw


def apply(obj, op, env):
    """Issue one operation; its output as bytes, or None."""
    name, a = op
    if env.kind == "ragged":
        assert name in RAGGED_ALLOWED, f"{name} aborts on a ragged ensemble by contract: the generator must never emit it"
    if name == "update":
        obj.update(a["n"], _dt(a, env))
    elif name == "step_async":
        dt = _dt(a, env)
        if env.members and not a.get("per_member"):
            dt = [dt] * env.members                  # an ensemble's async call takes an array: one value for all
        obj.step_async(a["n"], dt)                   # no sync: the next operation queues behind it
    elif name == "trace":
        return blob(obj.trace(a["n"], _dt(a, env), a["every"]))
    elif name == "update_adaptive":
        return adaptive_bits(obj.update_adaptive(a["n"], ETA, DT_MAX, **_adaptive_kw(a)))
    elif name == "update_adaptive_async":
        obj.update_adaptive_async(a["n"], ETA, DT_MAX, **_adaptive_kw(a))
    elif name == "adaptive_collect":
        return adaptive_bits(obj.adaptive_collect(a["n"]))
    elif name == "timestep":
        return struct.pack("<d", obj.timestep(ETA, DT_MAX))
    elif name == "energy":
        return ebits(obj.energy())
    elif name == "potential":
        return blob(obj.potential())
    elif name == "potential_at":
        return blob(obj.potential_at(env.points(a["count"]), SOFT))
    elif name == "acceleration_at":
        return blob(obj.acceleration_at(env.points(a["count"]), SOFT))
    elif name == "potential_map":
        return blob(obj.potential_map(env.view(a["w"], a["h"]), SOFT))
    elif name == "acceleration_map":
        return blob(obj.acceleration_map(env.view(a["w"], a["h"]), SOFT))
    elif name == "bounds":
        return blob(obj.bounds())
    elif name in ("render_counts", "render"):
        if "mode" in a:
            obj.render_mode(a["mode"])               # an ensemble's two render paths; the setting stays on the object
        return blob(getattr(obj, name)(env.view(a["w"], a["h"])))
    elif name == "get_data":
        return blob(obj.get_data())
    elif name == "get_member":
        return blob(obj.get_member(a["b"]))
    elif name == "set_data":
        obj.set_data(env.other)
    elif name == "sync":
        obj.sync()
    else:
        raise ValueError(f"unknown operation {name}")
    return None


# ---- the two runs --------------------------------------------------------------------------------------------------------------

def run_observed(make, ops, env):
    obj = make()
    obj.set_data(env.start)
    outs = [apply(obj, op, env) for op in ops]
    final = blob(obj.get_data())
    obj.close()
    return outs, final


def run_reference(make, ops, env):
    state, outs, collected = env.start, [], None
    for op in ops:
        if op[0] == "adaptive_collect":               # the fresh object that took the async call has collected already
            outs.append(collected)
            continue
        obj = make()
        obj.set_data(state)
        outs.append(apply(obj, op, env))
        if op[0] == "update_adaptive_async":
            collected = apply(obj, ("adaptive_collect", {"n": op[1]["n"]}), env)
        state = obj.get_data()
        obj.close()
    return outs, blob(state)


def check(make, ops, env, seed=None):
    """Raises SequenceMismatch naming the first operation whose output differs; returns the number of outputs compared."""
    got, got_final = run_observed(make, ops, env)
    want, want_final = run_reference(make, ops, env)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            what = "one of them returned nothing" if g is None or w is None else \
                f"{sum(x != y for x, y in zip(g, w)) + abs(len(g) - len(w))} of {len(w)} bytes"
            raise SequenceMismatch(seed, i, ops[i][0], ops, what)
    if got_final != want_final:
        raise SequenceMismatch(seed, len(ops), "final state", ops, "get_data after the last operation")
    return sum(g is not None for g in got) + 1


# ---- the generator -------------------------------------------------------------------------------------------------------------

def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _make(rng, kind, name, members):
    """One operation of that name with drawn arguments."""
    if name in ("update", "step_async"):
        a = {"n": int(_pick(rng, STEP_COUNTS)), "dt": float(_pick(rng, STEP_DTS))}
        if kind != "pipeline":
            a["per_member"] = bool(rng.random() < 0.5)
        return name, a
    if name == "trace":
        return name, {"n": int(_pick(rng, STEP_COUNTS)), "dt": float(_pick(rng, STEP_DTS)), "per_member": bool(rng.random() < 0.5),
                      "every": int(_pick(rng, TRACE_EVERY))}
    if name in ADAPTIVE:
        a = {"n": int(_pick(rng, ADAPT_COUNTS))}
        extra = rng.random()
        if extra < 0.25:
            a["span"] = ADAPT_SPAN
        elif extra < 0.45:
            a["prime"] = True
        return name, a
    if name in ("potential_at", "acceleration_at"):
        return name, {"count": int(_pick(rng, POINT_COUNTS))}
    if name in ("potential_map", "acceleration_map"):
        w, h = _pick(rng, MAP_SIZES)
        return name, {"w": w, "h": h}
    if name in ("render_counts", "render"):
        w, h = _pick(rng, RENDER_SIZES)
        a = {"w": w, "h": h}
        if kind == "batch":
            a["mode"] = int(rng.integers(2))
        return name, a
    if name == "get_member":
        return name, {"b": int(rng.integers(members))}
    return name, {}


def _flips(op):
    """how often the operation flips the position double buffer"""
    name, a = op
    return a["n"] + (1 if a.get("prime") else 0) if name in STEPPING else 0


def _segment(rng, kind, count, members):
    """`count` drawn operations.  After update_adaptive_async only operations that make no step follow until its
    adaptive_collect, which a stepping draw forces and the end of the segment forces at the latest."""
    step_w, rest_w = WEIGHTS[kind]
    names = list(step_w) + list(rest_w)
    p = np.array([step_w[n] for n in step_w] + [rest_w[n] for n in rest_w])
    p = p / p.sum()
    ops, waiting = [], None
    while len(ops) < count:
        name = names[int(rng.choice(len(names), p=p))]
        if waiting is not None and (name in STEPPING or rng.random() < 0.3):
            ops.append(("adaptive_collect", {"n": waiting}))
            waiting = None
            continue
        op = _make(rng, kind, name, members)
        ops.append(op)
        if name == "update_adaptive_async":
            waiting = op[1]["n"]
    if waiting is not None:
        ops.append(("adaptive_collect", {"n": waiting}))
    return ops


def generate(kind, seed, length=LENGTH, members=0):
    """The sequence of (kind, seed): drawn segments around four planted pieces, in this order --
      an odd call (adaptive where the kind has adaptive steps), so the phase bit flips;
      an async call with a diagnostic directly behind it;
      set_data in the middle (a single world: between two timestep() calls, the head armed before and asked after);
      a fixed-step call of >= 2 steps, which finds the chain cached for the other phase."""
    rng = np.random.default_rng(seed)
    if kind == "ragged":
        odd = ("update", {"n": 3, "dt": float(_pick(rng, STEP_DTS)), "per_member": True})
    else:
        odd = ("update_adaptive", {"n": int(_pick(rng, (1, 3)))})
    if kind == "pipeline" and rng.random() < 0.5:
        behind = [("update_adaptive_async", {"n": 3}), _make(rng, kind, _pick(rng, ("energy", "potential_map", "render")), members),
                  ("adaptive_collect", {"n": 3})]
    else:
        first = _make(rng, kind, "step_async", members)
        if kind != "pipeline":
            first[1]["per_member"] = True
        behind = [first, _make(rng, kind, _pick(rng, ("energy", "potential")), members)]
    middle = [("set_data", {})]
    if kind == "pipeline":
        middle = [("timestep", {}), ("set_data", {}), ("timestep", {})]
    chain = _make(rng, kind, "update", members)
    chain[1]["n"] = int(_pick(rng, (2, 7, 20)))
    planted = [[odd], behind, middle, [chain]]
    free = max(length - sum(len(p) for p in planted), 5)
    cuts = [free // 5 + (1 if i < free % 5 else 0) for i in range(5)]
    ops = []
    for i in range(5):
        ops += _segment(rng, kind, cuts[i], members)
        if i < 4:
            ops += planted[i]
    assert_covers(kind, ops)
    return ops


def assert_covers(kind, ops):
    """What every sequence must contain, asserted on the list itself: a change of weights cannot silently drop it."""
    names = [name for name, _ in ops]
    if kind == "ragged":
        assert set(names) <= RAGGED_ALLOWED, sorted(set(names) - RAGGED_ALLOWED)
    flipping = ADAPTIVE if kind != "ragged" else FIXED
    odd = [i for i, op in enumerate(ops) if op[0] in flipping and _flips(op) % 2 == 1]
    assert odd and any(op[0] in FIXED and op[1]["n"] >= 2 for op in ops[odd[0] + 1:]), \
        "no odd (adaptive) call with a fixed-step call of >= 2 steps after it"
    assert any(a in ASYNC and b in DIAGNOSTICS for a, b in zip(names, names[1:])), "no diagnostic directly after an async call"
    assert any(name == "set_data" and len(ops) // 4 <= i < len(ops) - len(ops) // 4 for i, name in enumerate(names)), \
        "no set_data in the middle"
    stepping = sum(name in STEPPING for name in names) / len(names)
    assert 0.2 <= stepping <= 0.5, f"{stepping:.2f} of the operations step: roughly every third should"
    waiting = None
    for name, a in ops:          # update_adaptive_async ... adaptive_collect pair up, with no step between them
        if name == "update_adaptive_async":
            assert waiting is None
            waiting = a["n"]
        elif name == "adaptive_collect":
            assert waiting == a["n"]
            waiting = None
        else:
            assert waiting is None or name not in STEPPING, f"{name} between update_adaptive_async and adaptive_collect"
    assert waiting is None
