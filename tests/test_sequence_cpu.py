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
(sequence_driver.assert_union_covers, at the member counts of the GPU rows) -- test_the_leapfrog_seeds_are_the_first_pair_that_catches_every_fault recomputes it.

The reads kinds ("pipeline-reads", "batch-reads", "ragged-reads"): the stand-in makes tidal_at, tidal_map, profile, pair_counts
and neighbours (an ensemble: the four Phi / g field calls too) through a model of the one ReadScratch they share (FakeReads): one
grow-only args array, one grow-only work array and one grow-only host array that KEEP their old contents, every call writing its
result into work in its own layout by merging -- pair counts and neighbour counts by addition, neighbour keys by minimum
(tests/paircount_ref.py and tests/neighbour_ref.py give the numbers) -- after resetting what it merges into, and a flag for the
interval.  bounds, render_counts and render go through the same three arrays -- the keys and the count image at the head of work,
where neighbour keys and pair tables lie too, a frame in a section behind its image -- inside an interval of their own
(FAULTS[27]: the image is not cleared).  READ_FAULTS plants one fault for each way of not doing so.  FakeBatch.ragged makes members of different sizes.  The
seeds of these kinds are chosen by the same procedure, with READ_FAULTS_OF for (a) and sequence_driver.assert_union_covers_reads
for (b); a single world is run in two environments, mixed and all massive, and a seed catches a fault if either run does --
test_the_reads_seeds_are_the_first_pair_that_catches_every_fault recomputes it."""
import hashlib
import itertools
import types

import numpy as np
import pytest

import neighbour_ref as nref
import paircount_ref as pref
import sequence_driver as sd

F32 = np.float32
MASK_OF = {name: mask for mask, name in nref.NAMES.items()}
N, M = 24, 13

FAULTS = {
    1: "after adaptive steps the next fixed-step call reuses the stale step size (dt_valid not cleared)",
    2: "a diagnostic, render or field call reads pos[cur ^ 1]",
    3: "the cached chain of phase 1 keeps the step size it was captured with",
    4: "a scratch buffer that regrew returns the old, shorter contents for the tail",
    5: "set_data leaves the adaptive head armed: the next criterion starts from the old minimum",
    6: "a diagnostic behind an async step sees the state before the step",
    7: "potential() after energy() returns the previous call's buffer",
    27: "render_counts adds into what the last read-only call left instead of clearing its image",
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


class ReadScratch:
    """nbody_amd/csrc/pipeline_internal.h ReadScratch as what it is: what a call uploads, what its kernels write, where the
    copied-back bytes land -- all three grow-only, all three KEEPING their old contents -- and whether the interval is valid."""

    def __init__(self):
        self.args, self.work, self.host = np.zeros(0, F32), np.zeros(0, np.uint8), np.zeros(0, np.uint8)
        self.uploaded, self.iv = -1, False          # the size of the last upload
        self.stride = 0                             # entries per member of the last call's layout; 0: packed at the offsets


def grown(buf, size):
    if buf.size >= size:
        return buf
    new = np.zeros(size, buf.dtype)
    new[:buf.size] = buf
    return new


def sample(comp, p, mass, at, soft):
    """Phi (comp 1), g (2) or the tidal tensor (3) of the sources (p, mass) at the points `at`, crude, float32 (k, comp)"""
    d = p[None, :, :].astype(np.float64) - at[:, None, :].astype(np.float64)
    r2 = (d * d).sum(axis=2) + soft
    if comp == 1:
        out = -(mass / np.sqrt(r2)).sum(axis=1)[:, None]
    elif comp == 2:
        out = (d * (mass / (r2 * np.sqrt(r2)))[:, :, None]).sum(axis=1)
    else:
        w3, w5 = mass / r2 ** 1.5, 3 * mass / r2 ** 2.5
        out = np.stack([(w5 * d[:, :, 0] ** 2 - w3).sum(axis=1), (w5 * d[:, :, 0] * d[:, :, 1]).sum(axis=1),
                        (w5 * d[:, :, 1] ** 2 - w3).sum(axis=1)], axis=1)
    return out.astype(F32)


def pixels(view):
    ys, xs = np.mgrid[0:view.height, 0:view.width]
    return np.stack([(xs.reshape(-1) + 0.5 - view.offset[0]) / view.zoom + view.target[0],
                     (ys.reshape(-1) + 0.5 - view.offset[1]) / view.zoom + view.target[1]], axis=1).astype(F32)


class FakeReads:
    """The read-only calls that go through one ReadScratch (self.read), for one world or an ensemble.  The owner gives
    _worlds(call) -> [(pos, vel, mass, mass_len) per member] and _out(arrays per member) -> the caller's shape.  Every call
    uploads its arguments into `args` and computes from what `args` then HOLDS, writes into `work` in its own layout over
    whatever is there -- pair counts and neighbour counts by adding, neighbour keys by minimum, after resetting what it merges
    into -- and the result is what comes back through `host`.  `fault` plants one entry of READ_FAULTS."""

    def _read_call(self, args, work_bytes, back_bytes, enqueue, render=False, at=0):
        """render: the call brackets the owner's render interval, not the scratch's; at: where in work the result starts"""
        r, up = self.read, None
        if args is not None:
            args = np.ascontiguousarray(args, dtype=F32).ravel()
            r.args = grown(r.args, args.size)
            if not (self.fault == 24 and args.size == r.uploaded):
                r.args[:args.size] = args
            r.uploaded = args.size
            up = r.args[:args.size]
        had = r.work.size
        r.work = grown(r.work, work_bytes)
        if render:
            self.render_iv = True
        else:
            r.iv = True
        enqueue(up, r.work)
        if self.fault == 25 and 0 < had < work_bytes:
            r.work[had:work_bytes] = 0               # the tail never arrives: what the new buffer held stays
        r.host = grown(r.host, back_bytes)
        r.host[:back_bytes] = r.work[at:at + back_bytes]
        return r.host[:back_bytes].copy()

    def _nothing(self, defaults):
        """a call with nothing to launch: the defaults, and the interval cleared"""
        r = self.read
        if self.fault != 21:
            r.iv = False
        if self.fault == 20:
            r.host = grown(r.host, defaults.size)
            return r.host[:defaults.size].copy()
        return defaults

    def last_diag_ms(self):
        return 1.0 if self.read.iv else 0.0

    def last_render_ms(self):
        return 1.0 if self.render_iv else 0.0

    # bounds, count images and frames: through the same scratch, inside the render interval.  The owner gives _seen() ->
    # [(pos, mass) per member] as a diagnostic finds them.
    def _bounds(self):
        """-> float32 (members, 4): minima and maxima taken into keys that are first set to their identities"""
        worlds = self._seen()
        nbytes = 16 * len(worlds)

        def enqueue(up, work):
            keys = work[:nbytes].view(F32).reshape(-1, 4)
            keys[:, 0:2], keys[:, 2:4] = np.inf, -np.inf
            for b, (p, _) in enumerate(worlds):
                keys[b, 0:2], keys[b, 2:4] = np.minimum(keys[b, 0:2], p.min(axis=0)), np.maximum(keys[b, 2:4], p.max(axis=0))
        return self._read_call(None, nbytes, nbytes, enqueue, render=True).view(F32).reshape(-1, 4)

    def _render(self, view, frame):
        """-> uint32 (members, 3, h, w), points ADDED into the image at the head of work; or, shaded from it into the section
        behind it, uint8 (members, h, w, 3)"""
        worlds = self._seen()
        shape = (len(worlds), 3, view.height, view.width)
        count_bytes = 4 * int(np.prod(shape))
        frame_bytes = count_bytes // 4 if frame else 0          # one byte per class and pixel

        def enqueue(up, work):
            img = work[:count_bytes].view(np.uint32).reshape(shape)
            if self.fault != 27:
                img[:] = 0
            for b, (p, mass) in enumerate(worlds):
                s = (p - np.asarray(view.target, F32)) * F32(view.zoom) + np.asarray(view.offset, F32)
                ok = (s[:, 0] >= 0) & (s[:, 0] < view.width) & (s[:, 1] >= 0) & (s[:, 1] < view.height)
                cls = np.where(mass <= 0, 0, np.where(mass < view.core_mass, 1, 2))
                np.add.at(img[b], (cls[ok], s[ok, 1].astype(np.int64), s[ok, 0].astype(np.int64)), 1)
            if frame:
                work[count_bytes:count_bytes + frame_bytes] = np.minimum(img.transpose(0, 2, 3, 1) * 80, 255).astype(np.uint8).ravel()
        if frame:
            back = self._read_call(None, count_bytes + frame_bytes, frame_bytes, enqueue, render=True, at=count_bytes)
            return back.reshape(shape[0], view.height, view.width, 3)
        return self._read_call(None, count_bytes, count_bytes, enqueue, render=True).view(np.uint32).reshape(shape)

    def _field(self, call, comp, pts, soft):
        """pts float32 (members, k, 2) -> float32 (members, k, comp)"""
        worlds = self._worlds(call)
        count, k = pts.shape[:2]
        nbytes = count * k * comp * 4
        self.read.stride = k
        if k == 0:
            return self._nothing(np.zeros(0, np.uint8)).view(F32).reshape(count, 0, comp)

        def enqueue(up, work):
            at, out = up.reshape(count, k, 2), work[:nbytes].view(F32).reshape(count, k, comp)
            for b, (pos, _, mass, m) in enumerate(worlds):
                out[b] = sample(comp, pos[:m], mass[:m], at[b], soft)
        return self._read_call(pts, nbytes, nbytes, enqueue).view(F32).reshape(count, k, comp)

    def _profile(self, edges, centres, weights):
        """centres float32 (members, 4) -> (float64 (members, bins + 2, 6), uint32 (members,))"""
        worlds = self._worlds("profile")
        e = np.asarray(edges, dtype=F32)
        count, rows = len(worlds), e.size + 1
        self.read.stride = rows
        table_bytes = count * rows * 6 * 8
        nbytes = table_bytes + 4 * count

        def enqueue(up, work):
            edge, c = up[:e.size].astype(np.float64), up[e.size:].reshape(count, 4).astype(np.float64)
            table, lost = work[:table_bytes].view(np.float64).reshape(count, rows, 6), work[table_bytes:nbytes].view(np.uint32)
            for b, (pos, vel, mass, m) in enumerate(worlds):
                top = m if weights == "mass" else pos.shape[0]
                w = mass[:top].astype(np.float64) if weights == "mass" else np.ones(top)
                d, u = pos[:top] - c[b, 0:2], vel[:top] - c[b, 2:4]
                r2 = (d * d).sum(axis=1)
                row = np.searchsorted(edge, np.sqrt(r2), side="right")
                table[b], lost[b] = 0.0, 0
                for col, v in enumerate((np.ones(top), w, w * r2, w * (d[:, 0] * u[:, 1] - d[:, 1] * u[:, 0]), w * (d * u).sum(axis=1),
                                         0.5 * w * (u * u).sum(axis=1))):
                    np.add.at(table[b, :, col], row, v)
        back = self._read_call(np.concatenate([e, np.asarray(centres, dtype=F32).ravel()]), nbytes, nbytes, enqueue)
        return back[:table_bytes].view(np.float64).reshape(count, rows, 6), back[table_bytes:].view(np.uint32)

    def _pair_counts(self, edges, classes):
        """-> (uint64 (members, bins + 2, 3), uint64 (members, 3)): tests/paircount_ref.py's model, ADDED into the table"""
        worlds = self._worlds("pair_counts")
        e = np.asarray(edges, dtype=F32)
        count, rows = len(worlds), e.size + 1
        mask = sum({"mm": pref.MM, "mt": pref.MT, "tt": pref.TT, "all": pref.ALL}[c] for c in ((classes,) if isinstance(classes, str) else classes))
        self.read.stride = rows
        table_bytes = count * rows * 3 * 8
        nbytes = table_bytes + count * 3 * 8

        def enqueue(up, work):
            table = work[:nbytes].view(np.uint64)
            if self.fault != 19:
                table[:] = 0
            out, lost = table[:count * rows * 3].reshape(count, rows, 3), table[count * rows * 3:].reshape(count, 3)
            for b, (pos, _, _, m) in enumerate(worlds):
                part = np.zeros((pos.shape[0], 8), F32)
                part[:, 0:2] = pos
                o, unplaced = pref.model(part, m, e, mask)
                out[b] += o
                lost[b] += unplaced
        back = self._read_call(None, nbytes, nbytes, enqueue).view(np.uint64)
        return back[:count * rows * 3].reshape(count, rows, 3), back[count * rows * 3:].reshape(count, 3)

    def _neighbours(self, radius, receivers, sources):
        """-> per member (q, index[, count]): tests/neighbour_ref.py's model, keys merged by minimum and counts by addition"""
        worlds = self._worlds("neighbours")
        sizes = [pos.shape[0] for pos, _, _, _ in worlds]
        true = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        # the packed layout: member b at its offset -- or, the planted fault, at the uniform stride the last call left behind
        stride = self.read.stride if self.fault == 26 and getattr(self, "is_ragged", False) else 0
        self.read.stride = 0
        at = [b * stride for b in range(len(sizes))] if stride else list(true[:-1])
        entries = max(int(true[-1]), at[-1] + sizes[-1])
        r, s = MASK_OF[receivers], MASK_OF[sources]
        counted = radius is not None
        back_bytes = entries * (12 if counted else 8)

        def spans(n, m):
            (r0, r1), (s0, s1) = nref.span(r, n, m), nref.span(s, n, m)
            return r1 > r0 and s1 > s0

        def enqueue(up, work):
            keys, counts = work[:entries * 8].view(np.uint64), work[entries * 8:entries * 12].view(np.uint32)
            if self.fault != 17:
                keys[:] = nref.KEY_NONE
            if counted and self.fault != 18:
                counts[:] = 0
            for b, (pos, _, _, m) in enumerate(worlds):
                part = np.zeros((sizes[b], 8), F32)
                part[:, 0:2] = pos
                q, index, cnt = nref.model(part, m, r, s, radius)
                key = np.where(index == nref.NONE, nref.KEY_NONE, (q.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64))
                sl = slice(at[b], at[b] + sizes[b])
                keys[sl] = np.minimum(keys[sl], key)
                if counted:
                    counts[sl] += cnt
        if any(spans(n, w[3]) for n, w in zip(sizes, worlds)):
            back = self._read_call(None, entries * 12, back_bytes, enqueue)
        else:
            defaults = np.zeros(back_bytes, np.uint8)
            defaults[:entries * 8] = 0xff
            back = self._nothing(defaults)
        keys = back[:entries * 8].view(np.uint64)
        index = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        q = np.where(index == nref.NONE, np.uint64(nref.INF_BITS), keys >> np.uint64(32)).astype(np.uint32).view(F32)
        out = (q, index, back[entries * 8:].view(np.uint32)) if counted else (q, index)
        return [tuple(a[true[b]:true[b + 1]].copy() for a in out) for b in range(len(sizes))]


class FakePipeline(FakeReads):
    """float32 Euler steps with the method names of nb.SimPipeline; `fault` plants one entry of FAULTS."""

    def __init__(self, n, m, fault=0):
        self.n, self.m, self.fault = n, m, fault
        self.read, self.render_iv = ReadScratch(), False
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
        self.read.iv = True
        self.phi, self.phi_fresh = self._phi(p, p, 1.0).astype(F32), True
        mass, v = self.mass.astype(np.float64), self.vel.astype(np.float64)
        mom = (mass[:, None] * v).sum(axis=0)
        with np.errstate(invalid="ignore"):          # a world of massless particles: 0 / 0, the same NaN every time
            com = (mass[:, None] * p).sum(axis=0) / mass.sum()
        return {"kinetic": float(0.5 * (mass * (v * v).sum(axis=1)).sum()), "potential": float(0.5 * (mass * self.phi).sum()),
                "mass": float(mass.sum()), "momentum": (float(mom[0]), float(mom[1])),
                "angular_momentum": float((mass * (p[:, 0] * v[:, 1] - p[:, 1] * v[:, 0])).sum()),
                "center_of_mass": (float(com[0]), float(com[1]))}

    def potential(self):
        p = self._latest().astype(np.float64)
        self.read.iv = True
        if not (self.fault == 7 and self.phi_fresh):
            self.phi = self._phi(p, p, 1.0).astype(F32)
        self.phi_fresh = False
        return self.phi.copy()

    def _into_scratch(self, values):
        """the result travels through the scratch buffer, which grows when a call needs more"""
        if values.size == 0:                                 # no probe: nothing to launch
            return self._nothing(np.zeros(0, np.uint8)).view(F32)
        self.read.iv = True
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

    def _seen(self):
        return [(self._latest(), self.mass)]

    def bounds(self):
        return self._bounds()[0]

    def render_counts(self, view):
        return self._render(view, False)[0]

    def render(self, view):
        return self._render(view, True)[0]

    # -- the calls of FakeReads, for one world ---------------------------------------------------------------------------
    def _state(self, call):
        """(pos, vel, mass, mass_len) as a call of FakeReads finds them"""
        if not (self.fault == 22 and call.startswith("tidal")):
            self._flush()
        pos = self.pos[self.cur ^ 1] if self.fault == 23 and call == "pair_counts" else self.pos[self.cur]
        return pos, self.vel, self.mass, self.m

    def _worlds(self, call):
        return [self._state(call)]

    def tidal_at(self, points, soft):
        return self._field("tidal_at", 3, np.asarray(points, dtype=F32)[None], soft)[0]

    def tidal_map(self, view, soft):
        return self._field("tidal_map", 3, pixels(view)[None], soft)[0].reshape(view.height, view.width, 3)

    def profile(self, edges, centre, centre_velocity, weights, return_unplaced):
        out, lost = self._profile(edges, np.concatenate([centre, centre_velocity])[None], weights)
        return out[0], int(lost[0])

    def pair_counts(self, edges, classes, return_unplaced):
        out, lost = self._pair_counts(edges, classes)
        return out[0], lost[0]

    def neighbours(self, radius, receivers, sources):
        return self._neighbours(radius, receivers, sources)[0]


class FakeBatch(FakeReads):
    """A list of FakePipeline members behind the method names of nb.SimBatch that the driver calls; step sizes one for all
    or one per member; trace records energy() rows."""

    def __init__(self, count, n, m, fault=0):
        self.members, self.fault, self.is_ragged = [FakePipeline(n, m, fault) for _ in range(count)], fault, False
        self.read, self.render_iv = ReadScratch(), False          # the ensemble's own: its reads are one launch for all members

    @classmethod
    def ragged(cls, sizes, mass_lens, fault=0):
        """members of different sizes (nb.SimBatch.ragged): lists of per-member arrays where a uniform ensemble stacks"""
        self = cls(0, 0, 0, fault)
        self.members, self.is_ragged = [FakePipeline(n, m, fault) for n, m in zip(sizes, mass_lens)], True
        return self

    def close(self):
        pass

    def _dts(self, dt):
        return [float(dt)] * len(self.members) if np.ndim(dt) == 0 else [float(x) for x in dt]

    def _out(self, per_member):
        return list(per_member) if self.is_ragged else np.stack(per_member)

    def set_data(self, a):
        for s, part in zip(self.members, a):
            s.set_data(part)

    def get_data(self):
        return self._out([s.get_data() for s in self.members])

    # -- the calls of FakeReads, one launch for all members -------------------------------------------------------------------
    def _worlds(self, call):
        return [s._state(call) for s in self.members]

    def _points(self, points):
        a = np.asarray(points, dtype=F32)
        return np.ascontiguousarray(np.broadcast_to(a, (len(self.members),) + a.shape) if a.ndim == 2 else a)

    def _pixels(self, views):
        views = views if isinstance(views, list) else [views] * len(self.members)
        return np.stack([pixels(v) for v in views]), views[0].height, views[0].width

    def potential_at(self, points, soft):
        return self._field("potential_at", 1, self._points(points), soft)[:, :, 0]

    def acceleration_at(self, points, soft):
        return self._field("acceleration_at", 2, self._points(points), soft)

    def tidal_at(self, points, soft):
        return self._field("tidal_at", 3, self._points(points), soft)

    def _map(self, call, comp, views, soft):
        pts, h, w = self._pixels(views)
        out = self._field(call, comp, pts, soft)
        return out.reshape((len(self.members), h, w) + ((comp,) if comp > 1 else ()))

    def potential_map(self, views, soft):
        return self._map("potential_map", 1, views, soft)

    def acceleration_map(self, views, soft):
        return self._map("acceleration_map", 2, views, soft)

    def tidal_map(self, views, soft):
        return self._map("tidal_map", 3, views, soft)

    def profile(self, edges, centre, centre_velocity, weights, return_unplaced):
        both = np.empty((len(self.members), 4), F32)
        both[:, 0:2], both[:, 2:4] = centre, centre_velocity
        return self._profile(edges, both, weights)

    def pair_counts(self, edges, classes, return_unplaced):
        return self._pair_counts(edges, classes)

    def neighbours(self, radius, receivers, sources):
        return tuple(self._out(list(arrays)) for arrays in zip(*self._neighbours(radius, receivers, sources)))

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
        self.read.iv = True
        return [s.energy() for s in self.members]

    def potential(self):
        self.read.iv = True
        return self._out([s.potential() for s in self.members])

    def _seen(self):
        return [s._seen()[0] for s in self.members]

    def bounds(self):
        return self._bounds()

    def render_mode(self, mode):
        self.mode = mode

    def render_counts(self, view):
        return self._render(view, False)

    def render(self, view):
        return self._render(view, True)


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
    if fault == 27:
        return first(lambda n, a: n in ("render_counts", "render"))          # a frame is shaded from the same image
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


# ---- the reads kinds ------------------------------------------------------------------------------------------------------------

READ_FAULTS = {
    17: "neighbours does not reset the keys it takes minima into",
    18: "neighbours with a radius does not zero the counts it adds into",
    19: "pair_counts does not zero the table it adds into",
    20: "a call with nothing to launch returns what the host vector already held instead of the defaults",
    21: "a call with nothing to launch leaves the interval valid",
    22: "tidal_at / tidal_map do not wait for queued async work",
    23: "pair_counts reads pos[cur ^ 1]",
    24: "an argument upload of the same size as the previous one is skipped: stale centres or probes",
    25: "a regrown work buffer returns the old, shorter contents for the tail of the call that grew it",
    26: "a member of a ragged ensemble is addressed with the uniform stride b * n the last call's layout left behind, not its offset",
}
# 20 shows only where a call that returns something has nothing to launch: neighbours in a world without a massless particle.
# The ensembles of the GPU rows have massless particles in some member, and so have these; 26 needs members of other sizes.
READ_FAULTS_OF = {"pipeline-reads": (17, 18, 19, 20, 21, 22, 23, 24, 25), "batch-reads": (17, 18, 19, 21, 22, 23, 24, 25),
                  "ragged-reads": (17, 18, 19, 21, 22, 23, 24, 25, 26)}
READS_MEMBERS = {"pipeline-reads": (0,), "batch-reads": (3, 5), "ragged-reads": (12,)}          # the member counts of the GPU rows
RAGGED_SIZES, RAGGED_MASS = [24, 1, 7, 13, 30, 9, 16, 2, 11, 5, 19, 3], [13, 1, 0, 13, 20, 1, 9, 1, 6, 2, 19, 2]


def world_of(n, m, seed):
    rng = np.random.default_rng([seed, n])
    a = np.zeros((n, 8), dtype=F32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 50
    a[:, 2:4] = rng.standard_normal((n, 2))
    a[:m, 7] = 1.5 + 3 * rng.random(m)
    a[m:, 7] = 0.5
    a[:m, 6] = 40 * a[:m, 7] ** 3
    return a


_probe_sets = np.random.default_rng(6).standard_normal((2, len(RAGGED_SIZES), max(sd.POINT_COUNTS), 2)).astype(F32) * 60


def read_points(members):
    def points(count, which=0, per_member=False):
        return _probe_sets[which][:members, :count] if per_member else _probe_sets[which][0, :count]
    return points


def read_view(w, h, b=None):
    v = view(w, h)
    if b is not None:
        v.target = (7.0 * b, -4.0 * b)
    return v


def read_edges(bins):
    return np.linspace(5.0, 150.0, bins + 1).astype(F32)


_CENTRES = (((3.0, -4.0), (0.5, -0.25)), ((-10.0, 6.0), (-1.0, 2.0)))


def read_centre(members):
    def centre(which, per_member=False):
        c, u = (np.array(x, dtype=F32) for x in _CENTRES[which])
        if not per_member:
            return c, u
        shift = np.arange(members, dtype=F32)[:, None]
        return c + 2 * shift, u - 0.125 * shift
    return centre


def reads_env(kind, start, other, members=0):
    return sd.Env(kind, start, other, read_view, read_points(members), members=members, edges=read_edges, centre=read_centre(members),
                  radius=30.0)


def reads_cases(kind, members):
    """[(environment, maker of the stand-in with a fault)] of a kind at a member count.  A single world runs twice: mixed, and --
    the classic row of the MI355X -- with every particle massive, where neighbours under EMPTY_MASKS has nothing to launch."""
    if kind == "pipeline-reads":
        return [(reads_env(kind, world(1), world(2)), lambda fault: (lambda: FakePipeline(N, M, fault))),
                (reads_env(kind, world_of(N, N, 3), world_of(N, N, 4)), lambda fault: (lambda: FakePipeline(N, N, fault)))]
    if kind == "batch-reads":
        env = reads_env(kind, np.stack([world(10 + b) for b in range(members)]), np.stack([world(20 + b) for b in range(members)]), members)
        return [(env, lambda fault: (lambda: FakeBatch(members, N, M, fault)))]
    sizes, masses = RAGGED_SIZES[:members], RAGGED_MASS[:members]
    env = reads_env(kind, [world_of(n, m, 30 + b) for b, (n, m) in enumerate(zip(sizes, masses))],
                    [world_of(n, m, 50 + b) for b, (n, m) in enumerate(zip(sizes, masses))], members)
    return [(env, lambda fault: (lambda: FakeBatch.ragged(sizes, masses, fault)))]


def reads_first_touch(fault, ops):
    """index of the first operation a fault of READ_FAULTS could change the output of"""
    def first(pred):
        return next(i for i, (n, a) in enumerate(ops) if pred(n, a))
    if fault in (17, 26):
        return first(lambda n, a: n == "neighbours")
    if fault == 18:
        return first(lambda n, a: n == "neighbours" and a["radius"])
    if fault in (19, 23):
        return first(lambda n, a: n == "pair_counts")
    if fault in (20, 21):
        return first(lambda n, a: n == "neighbours" or a.get("count") == 0)
    if fault == 22:
        return first(lambda n, a: n in sd.ASYNC)
    if fault == 24:
        return first(lambda n, a: n in sd.AT_CALLS + sd.MAP_CALLS + ("profile",))
    if fault == 25:          # whatever grows the work array: the renders too
        return first(lambda n, a: n in sd.DIAG_READS + ("bounds", "render_counts", "render"))
    raise ValueError(f"no first touch known for fault {fault}")


_reads_runs = {}


def reads_caught(kind, seed, fault, members):
    """None: the sequence passes in every environment of the kind; else the first SequenceMismatch.  Remembered: the seed
    search asks for every (seed, fault) once more."""
    key = (kind, seed, fault, members)
    if key not in _reads_runs:
        ops = sd.generate(kind, seed, members=members)
        _reads_runs[key] = None
        for env, maker in reads_cases(kind, members):
            try:
                sd.check(maker(fault), ops, env, seed)
            except sd.SequenceMismatch as e:
                _reads_runs[key] = e
                break
    return _reads_runs[key]


READS_ROWS = [(k, m) for k in sorted(READS_MEMBERS) for m in READS_MEMBERS[k]]


@pytest.mark.parametrize("kind,members", READS_ROWS)
def test_without_a_fault_every_committed_reads_seed_passes(kind, members):
    for seed in sd.SEEDS[kind]:
        ops = sd.generate(kind, seed, members=members)
        for env, maker in reads_cases(kind, members):
            assert sd.check(maker(0), ops, env, seed) > len(ops) // 2


@pytest.mark.parametrize("kind,fault", [(k, f) for k in sorted(READ_FAULTS_OF) for f in READ_FAULTS_OF[k]])
def test_every_planted_reads_fault_is_caught_by_a_committed_seed(kind, fault):
    members = READS_MEMBERS[kind][0]
    caught = []
    for seed in sd.SEEDS[kind]:
        e = reads_caught(kind, seed, fault, members)
        if e is not None:
            ops = sd.generate(kind, seed, members=members)
            assert e.seed == seed and e.index >= reads_first_touch(fault, ops), (READ_FAULTS[fault], e.index, reads_first_touch(fault, ops))
            assert e.name == (ops[e.index][0] if e.index < len(ops) else "final state")
            assert f"seed {seed}" in str(e) and sd.show(ops[0]) in str(e)
            caught.append(seed)
    assert caught, f"no committed seed of {kind} notices: {READ_FAULTS[fault]}"


@pytest.mark.parametrize("kind", ["pipeline-reads", "batch-reads"])
def test_a_render_that_does_not_clear_its_image_is_caught_by_a_committed_reads_seed(kind):
    """FAULTS[27], among reads that leave neighbour keys, pair tables and float maps where the image goes.  It is no entry of
    READ_FAULTS_OF: the seeds of the reads kinds were chosen before the renders went through the scratch."""
    members = READS_MEMBERS[kind][0]
    caught = []
    for seed in sd.SEEDS[kind]:
        e = reads_caught(kind, seed, 27, members)
        if e is not None:
            ops = sd.generate(kind, seed, members=members)
            assert e.seed == seed and e.index >= first_touch(27, ops) and e.name in ("render_counts", "render"), (e.index, e.name)
            caught.append(seed)
    assert caught, f"no committed seed of {kind} notices: {FAULTS[27]}"


def test_a_fault_a_kind_cannot_show_is_not_claimed():
    """20 on an ensemble with a massless particle somewhere, 26 on members of one size: the committed seeds pass, which is why
    READ_FAULTS_OF leaves them out"""
    for kind, fault in (("batch-reads", 20), ("batch-reads", 26), ("ragged-reads", 20), ("pipeline-reads", 26)):
        assert all(reads_caught(kind, seed, fault, READS_MEMBERS[kind][0]) is None for seed in sd.SEEDS[kind]), (kind, fault)


@pytest.mark.parametrize("kind", sorted(READ_FAULTS_OF))
def test_the_reads_seeds_are_the_first_pair_that_catches_every_fault(kind):
    """The rule of the module docstring for the reads kinds, recomputed; candidates that do not generate or do not pass clean
    are left out."""
    members = READS_MEMBERS[kind][0]
    catches = {}
    for seed in range(max(sd.SEEDS[kind]) + 1):
        try:
            if reads_caught(kind, seed, 0, members) is None:
                catches[seed] = {f for f in READ_FAULTS_OF[kind] if reads_caught(kind, seed, f, members) is not None}
        except AssertionError:
            continue          # assert_covers: this seed names no sequence

    def good(pair):
        if catches[pair[0]] | catches[pair[1]] != set(READ_FAULTS_OF[kind]):
            return False
        try:
            for count in READS_MEMBERS[kind]:
                sd.assert_union_covers_reads(kind, [sd.generate(kind, seed, members=count) for seed in pair])
        except AssertionError:
            return False
        return True
    pairs = (p for p in itertools.combinations(sorted(catches), 2) if good(p))
    assert next(pairs) == tuple(sd.SEEDS[kind]), {s: sorted(c) for s, c in catches.items()}


@pytest.mark.parametrize("kind,members", READS_ROWS)
def test_the_committed_reads_sequences_issue_every_operation_between_them(kind, members):
    sd.assert_union_covers_reads(kind, [sd.generate(kind, seed, members=members) for seed in sd.SEEDS[kind]])


@pytest.mark.parametrize("kind,members", READS_ROWS)
def test_committed_reads_sequences_hold_what_they_must(kind, members):
    for seed in sd.SEEDS[kind]:
        ops = sd.generate(kind, seed, members=members)
        sd.assert_covers(kind, ops)
        assert sd.READS_LENGTH <= len(ops) <= sd.READS_LENGTH + 4
        assert ops == sd.generate(kind, seed, members=members)          # a seed names one sequence
        names = {name for name, _ in ops}
        if kind == "ragged-reads":
            assert names <= sd.RAGGED_READS_ALLOWED and not names & {"bounds", "render", "render_counts", "update_adaptive", "timestep"}


def _without(ops, drop):
    """the list without the operations at which drop(i) holds"""
    return [op for i, op in enumerate(ops) if not drop(i)]


def test_the_generator_notices_a_dropped_reads_piece():
    ops = sd.generate("pipeline-reads", sd.SEEDS["pipeline-reads"][0])
    names = [name for name, _ in ops]

    def behind(first, family):
        return lambda i: i and names[i - 1] in first and sd.FAMILY.get(names[i]) == family
    for family in ("tidal", "profile", "pair_counts", "neighbours"):
        with pytest.raises(AssertionError, match=f"no {family} call directly behind step_async"):
            sd.assert_covers("pipeline-reads", _without(ops, behind(("step_async",), family)))
    with pytest.raises(AssertionError, match="update_adaptive_async"):
        sd.assert_covers("pipeline-reads", _without(ops, lambda i: i and names[i - 1] == "update_adaptive_async" and names[i] in sd.NEW_READS))

    def large(calls):          # the large call between the two small ones
        return lambda i: 0 < i < len(ops) - 1 and names[i] in calls and names[i - 1] == names[i] and ops[i - 1] == ops[i + 1]
    with pytest.raises(AssertionError, match="field call small, large"):
        sd.assert_covers("pipeline-reads", _without(ops, large(sd.AT_CALLS + sd.MAP_CALLS)))
    with pytest.raises(AssertionError, match="profile small, large"):
        sd.assert_covers("pipeline-reads", _without(ops, large(("profile",))))
    with pytest.raises(AssertionError, match=r"neighbours\(None\)"):
        sd.assert_covers("pipeline-reads", _without(ops, lambda i: 0 < i < len(ops) - 1 and names[i - 1] == names[i] == "neighbours" and
                                                    not ops[i][1]["radius"] and names[i + 1] == "pair_counts"))
    with pytest.raises(AssertionError, match="two pair_counts in a row"):
        sd.assert_covers("pipeline-reads", _without(ops, lambda i: i and names[i] == names[i - 1] == "pair_counts"))
    with pytest.raises(AssertionError, match="odd number of steps"):
        sd.assert_covers("pipeline-reads", _without(ops, lambda i: 0 < i < len(ops) - 1 and ops[i - 1] == ops[i + 1] and names[i] in sd.STEPPING))
    with pytest.raises(AssertionError, match="set_data"):
        sd.assert_covers("pipeline-reads", _without(ops, lambda i: names[i] == "set_data"))
    with pytest.raises(AssertionError, match="empty probe set"):
        sd.assert_covers("pipeline-reads", _without(ops, lambda i: ops[i][1].get("count") == 0))
    with pytest.raises(AssertionError, match="EMPTY_MASKS"):
        sd.assert_covers("pipeline-reads", _without(ops, lambda i: names[i] == "neighbours" and
                                                    (ops[i][1]["receivers"], ops[i][1]["sources"]) == sd.EMPTY_MASKS))
    ragged = sd.generate("ragged-reads", sd.SEEDS["ragged-reads"][0], members=12)
    with pytest.raises(AssertionError):
        sd.assert_covers("ragged-reads", ragged + [("bounds", {})])
    with pytest.raises(AssertionError, match="aborts on a ragged ensemble"):
        sd.apply(None, ("render", {"w": 32, "h": 18}), sd.Env("ragged-reads", None, None, None, None, members=12))


def test_the_interval_is_part_of_the_verdict():
    """a reads kind appends last_diag_ms() > 0 to the output of every call of DIAG_READS; an old kind does not"""
    env = reads_cases("pipeline-reads", 0)[0][0]
    s = FakePipeline(N, M)
    s.set_data(env.start)
    launched = sd.apply(s, ("tidal_at", {"count": 1, "which": 0}), env)
    assert len(launched) == 3 * 4 + 1 and launched[-1:] == b"\1"
    assert sd.apply(s, ("potential_at", {"count": 0, "which": 0}), env) == b"\0"
    for op in (("bounds", {}), ("render_counts", {"w": 32, "h": 18}), ("render", {"w": 32, "h": 18})):
        s.render_iv = False
        sd.apply(s, op, env)          # a render brackets an interval of its own and does not move that byte
        assert s.last_render_ms() > 0 and s.last_diag_ms() == 0
    assert len(sd.apply(s, ("potential_at", {"count": 1}), ENV)) == 4
