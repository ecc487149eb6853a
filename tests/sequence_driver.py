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

Leapfrog calls (the kinds "pipeline-lf" and "batch-lf").  A leapfrog call needs acc = F(x) of the state it starts from; an
object that does not know that to hold first runs one dt = 0 Euler step (the priming launch), and a fresh object never knows
it.  THE PREMISE: that launch computes `vel + acc * 0` and `pos + vel * 0`, which is the identity only where acc is finite
and no velocity or position is -0.0.  So the start state and the set_data state of these kinds must be finite and hold no
negative zero (assert_premise, called where the environments are built); then a long-lived object that rightly skips the
launch and a fresh one that makes it agree bit for bit, and one that skips it WRONGLY kicks with a stale acc and differs.
What bits cannot show -- a long-lived object that primes when it need not, and only wastes a force launch -- a second
oracle does: the driver keeps the one-bit model "acc is current" (true exactly after a leapfrog call, fixed or adaptive;
false after set_data, any Euler step and a trace of n > 0 steps) and compares last_leapfrog_info() of the observed object
with it directly after every leapfrog call: primed == not current, force launches == n + primed (the force evaluations of
the call, include/nbody_leapfrog.h: n + 1 for the first call of a sequence, n for every following one).

The reads kinds ("pipeline-reads", "batch-reads", "ragged-reads").  energy, potential, the six field calls, profile, pair_counts
and neighbours share one scratch and one host protocol (nbody_amd/csrc/pipeline_internal.h ReadScratch, read_call): two grow-only
device buffers, one grow-only host vector and one timed interval.  pair_counts adds into a table it must zero itself, neighbours
takes minima into keys it must set to all ones and adds into counts it must zero when a radius is given, and a call with nothing
to launch returns defaults and clears the interval.  A reads kind draws everything its base kind draws plus these calls (an
ensemble kind: the four Phi / g field calls too), with drawn arguments -- for an ensemble also whether points, views and centres
are one for all members or one per member -- and plants the pieces of _reads_pieces.  In these kinds the output of every call of
DIAG_READS is its bytes followed by ONE BYTE, last_diag_ms() > 0: "the interval was recorded by a call that launched and cleared
by one that did not" is part of the bitwise verdict, and no time is compared.

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
BINS = (4, 64)                    # profile and pair_counts: growing, too
PROFILE_WEIGHTS = ("mass", "number")
PAIR_CLASSES = (("mm",), ("mm", "mt"), "all")
MASKS = ("massive", "massless", "all")
EMPTY_MASKS = ("massless", "massless")          # nothing to launch in a world (or an ensemble) without a massless particle
LENGTH = 40
READS_LENGTH = 84                 # the reads kinds: about 40 planted operations and as many drawn ones
LF_LENGTH = 60                    # the leapfrog kinds: 40 and the planted leapfrog pieces
LONG_ADAPT = 70                   # > 64 logged steps: the adaptive head regrows (planted, "pipeline-lf" only)
# the committed seeds: tests/test_gpu_sequences.py runs exactly these, and tests/test_sequence_cpu.py shows that the
# "pipeline" ones catch every planted fault, and that each pair of the leapfrog kinds catches every leapfrog fault (and how
# those pairs were chosen), and each pair of the reads kinds every fault of the shared read scratch, chosen the same way
SEEDS ={"pipeline": (5, 8, 11), "batch": (5, 8), "ragged": (5, 8), "pipeline-lf": (0, 6), "batch-lf": (2, 3),
         "pipeline-reads": (0, 1), "batch-reads": (0, 1), "ragged-reads": (0, 1)}
BASE = {"pipeline-lf": "pipeline", "batch-lf": "batch"}          # a leapfrog kind draws everything its base kind draws
READS = {"pipeline-reads": "pipeline", "batch-reads": "batch", "ragged-reads": "ragged"}          # and so does a reads kind


def base_of(kind):
    return BASE.get(kind) or READS.get(kind, kind)

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
LEAPFROG = ("update_leapfrog", "update_leapfrog_async")
STEPPING = FIXED + ADAPTIVE + LEAPFROG
ASYNC = ("step_async", "update_adaptive_async", "update_leapfrog_async")
DIAGNOSTICS = ("energy", "potential", "potential_at", "acceleration_at", "potential_map", "acceleration_map", "bounds",
               "render_counts", "render")
AT_CALLS = ("potential_at", "acceleration_at", "tidal_at")
MAP_CALLS = ("potential_map", "acceleration_map", "tidal_map")
FAMILY = {"tidal_at": "tidal", "tidal_map": "tidal", "profile": "profile", "pair_counts": "pair_counts", "neighbours": "neighbours"}
NEW_READS = tuple(FAMILY)
# the calls of read_call: what last_diag_ms() speaks of
DIAG_READS = ("energy", "potential") + AT_CALLS[:2] + MAP_CALLS[:2] + NEW_READS
# of those, the ones that launch in every world of the rows whatever their drawn arguments (a probe set is never drawn empty)
LAUNCHED = tuple(n for n in DIAG_READS if n != "neighbours")

# name -> weight; the stepping operations of a kind sum to 1/3, everything else to 2/3
WEIGHTS = {
    "pipeline": ({"update": 0.12, "step_async": 0.07, "update_adaptive": 0.08, "update_adaptive_async": 0.06},
                 {"timestep": 0.06, "energy": 0.07, "potential": 0.06, "potential_at": 0.05, "acceleration_at": 0.05,
                  "potential_map": 0.05, "acceleration_map": 0.05, "bounds": 0.04, "render_counts": 0.05, "render": 0.06,
                  "get_data": 0.05, "set_data": 0.04, "sync": 0.04}),
    "batch": ({"update": 0.12, "step_async": 0.07, "update_adaptive": 0.08, "trace": 0.06},
              {"energy": 0.11, "potential": 0.10, "bounds": 0.07, "render_counts": 0.09, "render": 0.10, "get_data": 0.07,
               "get_member": 0.07, "set_data": 0.06}),
    # include/nbody_batch_ragged.h lists steps, trace, energy, potential, get and set, and the field, tidal, profile, pair-count and
    # neighbour calls, which this kind has never drawn ("ragged-reads" below does); render, bounds and adaptive calls abort on
    # a ragged ensemble by contract
    "ragged": ({"update": 0.15, "step_async": 0.10, "trace": 0.08},
               {"energy": 0.18, "potential": 0.17, "get_data": 0.12, "get_member": 0.10, "set_data": 0.10}),
    # the leapfrog kinds: the planted pieces are mostly steps, so the drawn segments step less often and the whole sequence
    # keeps "roughly every third operation steps"; the weights lowered most are those of the calls the planted pieces hold
    # many of (update, update_leapfrog), not those of the async calls
    "pipeline-lf": ({"update": 0.02, "step_async": 0.05, "update_adaptive": 0.03, "update_adaptive_async": 0.04,
                     "update_leapfrog": 0.02, "update_leapfrog_async": 0.03},
                    {"timestep": 0.06, "energy": 0.07, "potential": 0.06, "potential_at": 0.05, "acceleration_at": 0.05,
                     "potential_map": 0.05, "acceleration_map": 0.05, "bounds": 0.04, "render_counts": 0.05, "render": 0.06,
                     "get_data": 0.05, "set_data": 0.04, "sync": 0.04}),
    "batch-lf": ({"update": 0.02, "step_async": 0.05, "update_adaptive": 0.04, "trace": 0.02, "update_leapfrog": 0.02},
                 {"energy": 0.11, "potential": 0.10, "bounds": 0.07, "render_counts": 0.09, "render": 0.10, "get_data": 0.07,
                  "get_member": 0.07, "set_data": 0.06}),
    # the reads kinds: the steps of the base kind, and the new calls take about a third of the whole from the other calls
    "pipeline-reads": ({"update": 0.12, "step_async": 0.07, "update_adaptive": 0.08, "update_adaptive_async": 0.06},
                       {"timestep": 0.03, "energy": 0.04, "potential": 0.03, "potential_at": 0.03, "acceleration_at": 0.03,
                        "potential_map": 0.03, "acceleration_map": 0.03, "bounds": 0.02, "render_counts": 0.03, "render": 0.03,
                        "get_data": 0.04, "set_data": 0.03, "sync": 0.02, "tidal_at": 0.05, "tidal_map": 0.05, "profile": 0.06,
                        "pair_counts": 0.06, "neighbours": 0.08}),
    "batch-reads": ({"update": 0.12, "step_async": 0.07, "update_adaptive": 0.08, "trace": 0.06},
                    {"energy": 0.05, "potential": 0.05, "bounds": 0.03, "render_counts": 0.04, "render": 0.04, "get_data": 0.05,
                     "get_member": 0.04, "set_data": 0.04, "potential_at": 0.03, "acceleration_at": 0.03, "potential_map": 0.03,
                     "acceleration_map": 0.03, "tidal_at": 0.04, "tidal_map": 0.04, "profile": 0.05, "pair_counts": 0.05,
                     "neighbours": 0.06}),
    # include/nbody_batch_ragged.h: the above, and the field, tidal, profile, pair-count and neighbour calls (render, bounds and
    # adaptive calls still abort)
    "ragged-reads": ({"update": 0.15, "step_async": 0.10, "trace": 0.08},
                     {"energy": 0.07, "potential": 0.07, "get_data": 0.06, "get_member": 0.05, "set_data": 0.05, "potential_at": 0.03,
                      "acceleration_at": 0.03, "potential_map": 0.03, "acceleration_map": 0.03, "tidal_at": 0.04, "tidal_map": 0.04,
                      "profile": 0.06, "pair_counts": 0.06, "neighbours": 0.08}),
}
RAGGED_ALLOWED = frozenset(WEIGHTS["ragged"][0]) | frozenset(WEIGHTS["ragged"][1])
RAGGED_READS_ALLOWED = frozenset(WEIGHTS["ragged-reads"][0]) | frozenset(WEIGHTS["ragged-reads"][1])


def ragged_allowed(kind):
    return RAGGED_READS_ALLOWED if kind == "ragged-reads" else RAGGED_ALLOWED


class Env:
    """What a sequence runs on: the state it starts from, the state set_data brings in, the member count of an ensemble (0: a
    single world) and the factories that turn plain arguments into what the calls take; the states' scale is the test
    file's, not the driver's.  view(w, h) and points(count) serve the old kinds.  A reads kind also calls
      view(w, h, b)             member b's own view of that size
      points(count, which, per_member)
                                probe set 0 or 1: (count, 2), or (members, count, 2) with one set per member
      edges(bins)               bins + 1 radii for profile and pair_counts
      centre(which, per_member) (centre, centre velocity) 0 or 1, the velocity not zero: each (2,), or (members, 2)
      radius                    the finite radius of neighbours"""

    def __init__(self, kind, start, other, view, points, members=0, edges=None, centre=None, radius=None):
        self.kind, self.start, self.other, self.view, self.points, self.members = kind, start, other, view, points, members
        self.edges, self.centre, self.radius = edges, centre, radius


def assert_premise(*states):
    """The premise of the leapfrog kinds (module docstring): every value finite, no position or velocity -0.0."""
    for state in states:
        a = np.asarray(state, dtype=np.float32)
        assert np.isfinite(a).all(), "a state of a leapfrog sequence must be finite"
        moved = a[..., 0:4]
        assert not np.any((moved == 0) & np.signbit(moved)), "a state of a leapfrog sequence must hold no -0.0 position or velocity"


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
    if args.get("leapfrog"):
        kw["leapfrog"] = True
    return kw


def _probes(a, env):
    if "which" not in a:
        return env.points(a["count"])
    return env.points(a["count"], a["which"], bool(a.get("per_member")))


def _views(a, env):
    if a.get("per_member"):
        return [env.view(a["w"], a["h"], b) for b in range(env.members)]
    return env.view(a["w"], a["h"])


def _read(obj, name, a, env):
    """one of the calls the reads kinds add, with the arguments the environment makes of the drawn ones"""
    if name == "tidal_at":
        return obj.tidal_at(_probes(a, env), SOFT)
    if name == "tidal_map":
        return obj.tidal_map(_views(a, env), SOFT)
    if name == "profile":
        centre, velocity = env.centre(a["centre"], bool(a.get("per_member")))
        return obj.profile(env.edges(a["bins"]), centre, velocity, a["weights"], return_unplaced=True)
    if name == "pair_counts":
        return obj.pair_counts(env.edges(a["bins"]), classes=a["classes"], return_unplaced=True)
    return obj.neighbours(env.radius if a["radius"] else None, a["receivers"], a["sources"])


def apply(obj, op, env):
    """Issue one operation; its output as bytes, or None.  A reads kind: the interval's byte behind every call of DIAG_READS."""
    out = _apply(obj, op, env)
    if env.kind in READS and op[0] in DIAG_READS:
        out += b"\1" if obj.last_diag_ms() > 0 else b"\0"
    return out


def _apply(obj, op, env):
    name, a = op
    if base_of(env.kind) == "ragged":
        assert name in ragged_allowed(env.kind), f"{name} aborts on a ragged ensemble by contract: the generator must never emit it"
    if name == "update":
        obj.update(a["n"], _dt(a, env))
    elif name == "step_async":
        dt = _dt(a, env)
        if env.members and not a.get("per_member"):
            dt = [dt] * env.members                  # an ensemble's async call takes an array: one value for all
        obj.step_async(a["n"], dt)                   # no sync: the next operation queues behind it
    elif name == "update_leapfrog":
        obj.update_leapfrog(a["n"], _dt(a, env))
    elif name == "update_leapfrog_async":
        obj.update_leapfrog_async(a["n"], a["dt"])   # a single world only: a SimBatch has no async form
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

def is_leapfrog(op):
    return op[0] in LEAPFROG or (op[0] in ADAPTIVE and bool(op[1].get("leapfrog")))


def acc_model(current, op):
    """The one-bit model "acc is current" after `op` (module docstring)."""
    name, a = op
    if is_leapfrog(op):
        return True
    if name == "set_data" or (name in STEPPING and a["n"] > 0):
        return False
    return current


def run_observed(make, ops, env, seed=None):
    obj = make()
    obj.set_data(env.start)
    if env.kind not in BASE:
        outs = [apply(obj, op, env) for op in ops]
    else:
        outs, current = [], False
        for i, op in enumerate(ops):
            outs.append(apply(obj, op, env))
            if is_leapfrog(op):              # read now: any later call may overwrite it
                want, got = (op[1]["n"] + (not current), not current), tuple(obj.last_leapfrog_info())
                if got != want:
                    raise SequenceMismatch(seed, i, op[0], ops, f"last_leapfrog_info() is (force launches, primed) = {got}, "
                                           f"the model of 'acc is current' says {want}")
            current = acc_model(current, op)
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
    got, got_final = run_observed(make, ops, env, seed)
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
    base = base_of(kind)
    if kind in READS and name in DIAG_READS:
        return _make_read(rng, name, base != "pipeline")
    if name in ("update", "step_async", "update_leapfrog", "update_leapfrog_async"):
        a = {"n": int(_pick(rng, STEP_COUNTS)), "dt": float(_pick(rng, STEP_DTS))}
        if base != "pipeline":
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
        if kind in BASE and rng.random() < 0.5:          # prime may come with it: the library ignores it under leapfrog
            a["leapfrog"] = True
        return name, a
    if name in ("potential_at", "acceleration_at"):
        return name, {"count": int(_pick(rng, POINT_COUNTS))}
    if name in ("potential_map", "acceleration_map"):
        w, h = _pick(rng, MAP_SIZES)
        return name, {"w": w, "h": h}
    if name in ("render_counts", "render"):
        w, h = _pick(rng, RENDER_SIZES)
        a = {"w": w, "h": h}
        if base == "batch":
            a["mode"] = int(rng.integers(2))
        return name, a
    if name == "get_member":
        return name, {"b": int(rng.integers(members))}
    return name, {}


def _make_read(rng, name, ensemble):
    """A call of DIAG_READS in a reads kind: every argument drawn; an ensemble also draws one for all / one per member."""
    if name in AT_CALLS:
        a = {"count": int(_pick(rng, POINT_COUNTS)), "which": int(rng.integers(2))}
    elif name in MAP_CALLS:
        w, h = _pick(rng, MAP_SIZES)
        a = {"w": w, "h": h}
    elif name == "profile":
        a = {"bins": int(_pick(rng, BINS)), "weights": _pick(rng, PROFILE_WEIGHTS), "centre": int(rng.integers(2))}
    elif name == "pair_counts":
        return name, {"bins": int(_pick(rng, BINS)), "classes": _pick(rng, PAIR_CLASSES)}
    elif name == "neighbours":
        return name, {"radius": bool(rng.random() < 0.5), "receivers": _pick(rng, MASKS), "sources": _pick(rng, MASKS)}
    else:
        return name, {}
    if ensemble:
        a["per_member"] = bool(rng.random() < 0.5)
    return name, a


def _flips(op):
    """how often the operation flips the position double buffer"""
    name, a = op
    return a["n"] + (1 if a.get("prime") and not a.get("leapfrog") else 0) if name in STEPPING else 0


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


def _leapfrog_pieces(rng, kind, members):
    """The planted pieces of the leapfrog kinds, four groups that share their leapfrog calls (lf: a fixed leapfrog call):
      step_async, lf, lf, update(dt X), lf, update(>= 2 steps, dt X)
                                           a leapfrog call queued behind async steps: the step word is zeroed behind a chain
                                           that still reads it; two in a row -- the second must not prime; an Euler update between two; after the
                                           third the step word holds 0 while the host last uploaded X, and the chain of that
                                           phase may be cached
      lf, set_data, lf [, trace, lf]       set_data between two; an ensemble: a trace of n > 0 steps between two
      adaptive(70 steps), lf_async, read   a single world: the head regrows with the kick words inside it, somewhere before
                                           a leapfrog call; an async leapfrog call with a diagnostic, map or render behind it
      adaptive leapfrog(2), adaptive leapfrog(1), lf
                                           the first leaves its last step size in kick word 1 and closes with it; the second
                                           (odd n) must close with word (n - 1) & 1 = 0, the row the fixed call then writes"""
    def lf():
        return _make(rng, kind, "update_leapfrog", members)
    used = _make(rng, kind, "update", members)
    if "per_member" in used[1]:
        used[1]["per_member"] = False      # one step size for all: the one the host remembers
    again = ("update", dict(used[1], n=int(_pick(rng, (2, 7, 20)))))
    between = [lf(), ("set_data", {}), lf()]
    if kind == "batch-lf":
        between += [_make(rng, kind, "trace", members), lf()]
    regrow = []
    if kind == "pipeline-lf":
        long_call = ("update_adaptive", {"n": LONG_ADAPT})
        if rng.random() < 0.5:
            long_call[1]["leapfrog"] = True
        regrow = [long_call, _make(rng, kind, "update_leapfrog_async", members),
                  _make(rng, kind, _pick(rng, ("energy", "potential_map", "render")), members)]
    closing = [("update_adaptive", {"n": 2, "leapfrog": True}), ("update_adaptive", {"n": 1, "leapfrog": True}), lf()]
    queued = _make(rng, kind, "step_async", members)          # drawn last: the draws of the pieces above stay where they were
    return [[queued, lf(), lf(), used, lf(), again], between, regrow, closing]


def generate(kind, seed, length=None, members=0):
    """The sequence of (kind, seed): drawn segments around four planted pieces, in this order --
      an odd call (adaptive where the kind has adaptive steps), so the phase bit flips;
      an async call with a diagnostic directly behind it;
      set_data in the middle (a single world: between two timestep() calls, the head armed before and asked after);
      a fixed-step call of >= 2 steps, which finds the chain cached for the other phase.
    The leapfrog kinds plant the four groups of _leapfrog_pieces between them."""
    if kind in BASE:
        return _generate_leapfrog(kind, seed, LF_LENGTH if length is None else length, members)
    if kind in READS:
        return _generate_reads(kind, seed, READS_LENGTH if length is None else length, members)
    length = LENGTH if length is None else length
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


def _generate_leapfrog(kind, seed, length, members):
    rng = np.random.default_rng([seed, len(kind)])          # a stream of its own: the base kind's seeds name other lists
    base = BASE[kind]
    odd = ("update_adaptive", {"n": int(_pick(rng, (1, 3)))})
    if base == "pipeline" and rng.random() < 0.5:
        behind = [("update_adaptive_async", {"n": 3}), _make(rng, kind, _pick(rng, ("energy", "potential_map", "render")), members),
                  ("adaptive_collect", {"n": 3})]
    else:
        first = _make(rng, kind, "step_async", members)
        if base != "pipeline":
            first[1]["per_member"] = True
        behind = [first, _make(rng, kind, _pick(rng, ("energy", "potential")), members)]
    middle = [("timestep", {}), ("set_data", {}), ("timestep", {})] if base == "pipeline" else [("set_data", {})]
    chain = _make(rng, kind, "update", members)
    chain[1]["n"] = int(_pick(rng, (2, 7, 20)))
    rows, between, regrow, closing = _leapfrog_pieces(rng, kind, members)
    planted = [p for p in ([odd], rows, behind, between, middle, regrow, closing, [chain]) if p]
    gaps = len(planted) + 1
    free = max(length - sum(len(p) for p in planted), gaps)
    ops = []
    for i in range(gaps):
        ops += _segment(rng, kind, free // gaps + (1 if i < free % gaps else 0), members)
        if i < len(planted):
            ops += planted[i]
    assert_covers(kind, ops)
    return ops


def _sized(op, size):
    """the same call at the smallest (0) or the largest (-1) drawn size"""
    name, a = op
    a = dict(a)
    if name in AT_CALLS:
        a["count"] = POINT_COUNTS[size]
    elif name in MAP_CALLS:
        a["w"], a["h"] = MAP_SIZES[size]
    else:
        a["bins"] = BINS[size]
    return name, a


def _size(op):
    name, a = op
    return a["count"] if name in AT_CALLS else a["w"] * a["h"] if name in MAP_CALLS else a["bins"] if "bins" in a else None


def _reads_pieces(rng, kind, members, odd, middle):
    """The planted pieces of the reads kinds (R: one of NEW_READS; the two R of a piece are the same call):
      step_async, R                 four times, one R of each family (tidal, profile, pair_counts, neighbours): a read queues
                                    behind async steps and sees the state after them
      update_adaptive_async, R, adaptive_collect
                                    a single world: the same behind the adaptive async call
      field(small), field(large), field(small); profile(4 bins), profile(64), profile(4)
                                    grow and shrink: the second small call runs inside buffers larger than it needs, over
                                    what the large one left
      neighbours(radius, A, B), neighbours(None, C, D), pair_counts, neighbours(radius, C, D)   with (A, B) != (C, D)
                                    the counts of the first call lie where the last one adds; the call between them with no
                                    radius must not have touched them, the table of pair_counts lies over the keys
      pair_counts, pair_counts      other classes: a table that is not zeroed keeps the first call's columns
      R, an odd number of steps, R  the phase bit flips between them (`odd`: the base kind's odd call)
      R, set_data, R                (`middle`: the base kind's set_data piece)
      X, potential_at(no points), Y; X, neighbours(EMPTY_MASKS), Y
                                    nothing to launch -- always for an empty probe set, and for these masks where no member has a
                                    massless particle -- between two reads of LAUNCHED: defaults come back, the interval is
                                    cleared, and neither the scratch nor the host vector is what the next call may rest on"""
    ensemble = base_of(kind) != "pipeline"

    def mk(name):
        return _make(rng, kind, name, members)

    def queued():
        op = mk("step_async")
        if ensemble:
            op[1]["per_member"] = True
        return op
    behind = [[queued(), mk(_pick(rng, fam))] for fam in (("tidal_at", "tidal_map"), ("profile",), ("pair_counts",), ("neighbours",))]
    if not ensemble:
        behind.append([("update_adaptive_async", {"n": 3}), mk(_pick(rng, NEW_READS)), ("adaptive_collect", {"n": 3})])
    field = mk(_pick(rng, AT_CALLS + MAP_CALLS))
    prof = mk("profile")
    grow = [[_sized(field, 0), _sized(field, -1), _sized(field, 0)], [_sized(prof, 0), _sized(prof, -1), _sized(prof, 0)]]
    first = (_pick(rng, MASKS), _pick(rng, MASKS))
    second = first
    while second == first:
        second = (_pick(rng, MASKS), _pick(rng, MASKS))

    def neigh(radius, masks):
        return "neighbours", {"radius": radius, "receivers": masks[0], "sources": masks[1]}
    c1 = int(rng.integers(len(PAIR_CLASSES)))
    c2 = (c1 + 1 + int(rng.integers(len(PAIR_CLASSES) - 1))) % len(PAIR_CLASSES)
    bins = int(_pick(rng, BINS))
    accumulate = [[neigh(True, first), neigh(False, second), mk("pair_counts"), neigh(True, second)],
                  [("pair_counts", {"bins": bins, "classes": PAIR_CLASSES[c1]}), ("pair_counts", {"bins": bins, "classes": PAIR_CLASSES[c2]})]]
    r1, r2 = mk(_pick(rng, NEW_READS)), mk(_pick(rng, NEW_READS))
    phase = [[r1, odd, (r1[0], dict(r1[1]))], [r2] + middle + [(r2[0], dict(r2[1]))]]
    no_points = {"count": 0, "which": 0}
    if ensemble:
        no_points["per_member"] = False
    nothing = [[mk(_pick(rng, [n for n in LAUNCHED if n != "potential_at"])), ("potential_at", no_points), mk(_pick(rng, [n for n in LAUNCHED if n != "potential_at"]))],
               [mk(_pick(rng, LAUNCHED)), neigh(bool(rng.random() < 0.5), EMPTY_MASKS), mk(_pick(rng, LAUNCHED))]]
    return behind, grow, accumulate, phase, nothing


def _generate_reads(kind, seed, length, members):
    rng = np.random.default_rng([seed, len(kind), 1])          # a stream of its own: no list of another kind moves
    base = READS[kind]
    if base == "ragged":
        odd = ("update", {"n": 3, "dt": float(_pick(rng, STEP_DTS)), "per_member": True})
    else:
        odd = ("update_adaptive", {"n": int(_pick(rng, (1, 3)))})
    first = _make(rng, kind, "step_async", members)
    if base != "pipeline":
        first[1]["per_member"] = True
    old_behind = [first, _make(rng, kind, _pick(rng, ("energy", "potential")), members)]
    middle = [("timestep", {}), ("set_data", {}), ("timestep", {})] if base == "pipeline" else [("set_data", {})]
    chain = _make(rng, kind, "update", members)
    chain[1]["n"] = int(_pick(rng, (2, 7, 20)))
    behind, grow, accumulate, phase, nothing = _reads_pieces(rng, kind, members, odd, middle)
    # the odd call first and the chain last (the base kind's order), set_data in the middle
    planted = [phase[0]] + behind[:4] + [grow[0], accumulate[0]] + behind[4:] + [phase[1], grow[1], accumulate[1]] + nothing + [old_behind, [chain]]
    gaps = len(planted) + 1
    free = max(length - sum(len(p) for p in planted), gaps)
    ops = []
    for i in range(gaps):
        ops += _segment(rng, kind, free // gaps + (1 if i < free % gaps else 0), members)
        if i < len(planted):
            ops += planted[i]
    assert_covers(kind, ops)
    return ops


def _same_around(ops, inner, outer=lambda op: op[0] in NEW_READS):
    """is there a call `outer` accepts, then one or more operations that `inner` accepts as a list, then the very same call?"""
    for i, op in enumerate(ops):
        if outer(op):
            for j in range(i + 2, len(ops)):
                if ops[j] == op and inner(ops[i + 1:j]):
                    return True
    return False


def assert_covers_reads(kind, ops):
    """The planted pieces of the reads kinds (_reads_pieces), on the list itself."""
    pairs = list(zip(ops, ops[1:]))
    for family in sorted(set(FAMILY.values())):
        assert any(a[0] == "step_async" and FAMILY.get(b[0]) == family for a, b in pairs), f"no {family} call directly behind step_async"
    if READS[kind] == "pipeline":
        assert any(a[0] == "update_adaptive_async" and b[0] in NEW_READS for a, b in pairs), "no new read directly behind update_adaptive_async"

    def grows(names):
        return any(a == c and a[0] == b[0] and a[0] in names and _size(a) == _size(_sized(a, 0)) and _size(b) == _size(_sized(a, -1))
                   for a, b, c in zip(ops, ops[1:], ops[2:]))
    assert grows(AT_CALLS + MAP_CALLS), "no field call small, large and small again"
    assert grows(("profile",)), "no profile small, large and small again"

    def neigh(op, radius):
        return op[0] == "neighbours" and op[1]["radius"] == radius

    def masks(op):
        return op[1]["receivers"], op[1]["sources"]
    assert any(neigh(a, True) and neigh(b, False) and c[0] == "pair_counts" and neigh(d, True) and masks(b) == masks(d) != masks(a)
               for a, b, c, d in zip(ops, ops[1:], ops[2:], ops[3:])), \
        "no neighbours(radius), neighbours(None) under other masks, pair_counts, neighbours(radius) under those masks"
    assert any(a[0] == b[0] == "pair_counts" and a[1]["classes"] != b[1]["classes"] for a, b in pairs), "no two pair_counts in a row with other classes"
    assert _same_around(ops, lambda inner: len(inner) == 1 and inner[0][0] in STEPPING and _flips(inner[0]) % 2 == 1), \
        "no new read before and after an odd number of steps"
    assert _same_around(ops, lambda inner: any(op[0] == "set_data" for op in inner) and all(op[0] in ("set_data", "timestep") for op in inner)), \
        "no new read before and after set_data"

    def launched(op, but):
        return op[0] in LAUNCHED and op[0] != but and _size(op) != 0
    assert any(launched(a, "potential_at") and b[0] == "potential_at" and b[1]["count"] == 0 and launched(c, "potential_at")
               for a, b, c in zip(ops, ops[1:], ops[2:])), "no empty probe set between two launched reads of another kind"
    assert any(launched(a, "neighbours") and b[0] == "neighbours" and masks(b) == EMPTY_MASKS and launched(c, "neighbours")
               for a, b, c in zip(ops, ops[1:], ops[2:])), "no neighbours under EMPTY_MASKS between two launched reads of another kind"


def assert_union_covers_reads(kind, lists):
    """What the committed sequences of a reads kind must hold BETWEEN them: every operation the kind draws, neighbours with and
    without a radius, and each ensemble argument (points, views, centres) one for all and one per member."""
    ops = [op for lst in lists for op in lst]
    names = {name for name, _ in ops}
    every = set(WEIGHTS[kind][0]) | set(WEIGHTS[kind][1])
    assert every <= names, f"the committed {kind} sequences never issue {sorted(every - names)}"
    for radius in (True, False):
        assert any(n == "neighbours" and a["radius"] == radius for n, a in ops), f"no neighbours with radius {radius}"
    if READS[kind] != "pipeline":
        for what, calls in (("points", AT_CALLS), ("views", MAP_CALLS), ("centres", ("profile",))):
            for per_member in (True, False):
                assert any(n in calls and a.get("count") != 0 and a["per_member"] == per_member for n, a in ops), \
                    f"no {what} {'one per member' if per_member else 'one for all'}"


def _between_leapfrog(ops, inner):
    """is there a leapfrog call, then exactly the operations `inner` accepts (one predicate each), then a leapfrog call?"""
    k = len(inner)
    return any(is_leapfrog(ops[i]) and is_leapfrog(ops[i + k + 1]) and all(f(*ops[i + 1 + j]) for j, f in enumerate(inner))
               for i in range(len(ops) - k - 1))


def assert_covers_leapfrog(kind, ops):
    """The planted leapfrog pieces, on the list itself."""
    names = [name for name, _ in ops]
    assert _between_leapfrog(ops, []), "no two leapfrog calls in a row"
    assert any(a[0] == "step_async" and is_leapfrog(b) for a, b in zip(ops, ops[1:])), "no leapfrog call directly behind step_async"
    assert _between_leapfrog(ops, [lambda n, a: n == "update" and a["n"] > 0]), "no Euler update between two leapfrog calls"
    assert _between_leapfrog(ops, [lambda n, a: n == "set_data"]), "no set_data between two leapfrog calls"
    if kind == "batch-lf":
        assert _between_leapfrog(ops, [lambda n, a: n == "trace" and a["n"] > 0]), "no trace of n > 0 steps between two leapfrog calls"
        assert "update_leapfrog_async" not in names, "a SimBatch has no async leapfrog call"

    def one_for_all(a):
        return not a.get("per_member")
    used = set()
    stale_word = False
    for i, (name, a) in enumerate(ops):
        if name == "update" and a["n"] >= 2 and one_for_all(a) and a["dt"] in used and i > 0 and is_leapfrog(ops[i - 1]):
            stale_word = True
        if name in ("update", "step_async", "trace") and one_for_all(a):
            used.add(a["dt"])
    assert stale_word, "no leapfrog call followed by a fixed-step update of >= 2 steps with a step size used before"
    assert any(n == "update_adaptive" and a.get("leapfrog") and a["n"] % 2 == 1 and ops[i + 1][0] in LEAPFROG
               for i, (n, a) in enumerate(ops[:-1])), "no adaptive leapfrog call of odd n followed by a fixed leapfrog call"
    if kind == "pipeline-lf":
        assert any(a == "update_leapfrog_async" and b in DIAGNOSTICS for a, b in zip(names, names[1:])), \
            "no diagnostic, map or render directly behind update_leapfrog_async"
        grown = [i for i, (n, a) in enumerate(ops) if n in ADAPTIVE and a["n"] > 64]
        assert grown and any(is_leapfrog(op) for op in ops[grown[0] + 1:]), "no adaptive call of > 64 steps before a leapfrog call"
    assert not any(a.get("resume") for _, a in ops), "resume=True: a fresh object cannot continue a clock"


def assert_union_covers(kind, lists):
    """What the committed sequences of a leapfrog kind must hold BETWEEN them: every operation the kind draws, and the adaptive
    calls in each drawn form.  The seeds are chosen so that this holds (tests/test_sequence_cpu.py)."""
    ops = [op for lst in lists for op in lst]
    names = {name for name, _ in ops}
    every = set(WEIGHTS[kind][0]) | set(WEIGHTS[kind][1])
    assert every <= names, f"the committed {kind} sequences never issue {sorted(every - names)}"
    for what in ("span", "prime", "leapfrog"):
        assert any(n in ADAPTIVE and a.get(what) for n, a in ops), f"no adaptive call with {what}"
    assert any(n in ADAPTIVE and a.get("prime") and a.get("leapfrog") for n, a in ops), "no adaptive leapfrog call with prime"
    if kind == "pipeline-lf":
        assert any(n == "update_adaptive_async" and a.get("leapfrog") for n, a in ops), "no async adaptive leapfrog call"


def assert_covers(kind, ops):
    """What every sequence must contain, asserted on the list itself: a change of weights cannot silently drop it."""
    names = [name for name, _ in ops]
    lf = kind in BASE
    if lf:
        assert_covers_leapfrog(kind, ops)
        kind = BASE[kind]
    allowed = ragged_allowed(kind)
    if kind in READS:
        assert_covers_reads(kind, ops)
        kind = READS[kind]
    if kind == "ragged":
        assert set(names) <= allowed, sorted(set(names) - allowed)
    flipping = ADAPTIVE if kind != "ragged" else FIXED
    odd = [i for i, op in enumerate(ops) if op[0] in flipping and _flips(op) % 2 == 1]
    assert odd and any(op[0] in FIXED and op[1]["n"] >= 2 for op in ops[odd[0] + 1:]), \
        "no odd (adaptive) call with a fixed-step call of >= 2 steps after it"
    assert any(a in ASYNC and b in DIAGNOSTICS for a, b in zip(names, names[1:])), "no diagnostic directly after an async call"
    assert any(name == "set_data" and len(ops) // 4 <= i < len(ops) - len(ops) // 4 for i, name in enumerate(names)), \
        "no set_data in the middle"
    stepping = sum(name in STEPPING for name in names) / len(names)
    most = 0.42 if lf else 0.5          # the leapfrog kinds plant many steps: hold them nearer to a third, seed by seed
    assert 0.2 <= stepping <= most, f"{stepping:.2f} of the operations step: roughly every third should"
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
