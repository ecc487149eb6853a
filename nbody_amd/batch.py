"""SimBatch: the ensembles of include/nbody_hip.h (nb_hip_batch_*, nb_hip_ragged_*, nb_hip_ensemble_*), and what every ensemble
class needs to pack members and step sizes."""
import ctypes as C

import numpy as np

from ._abi import NbAdaptiveResult, adaptive_cfg, as_ensemble, as_particles, hip_lib
from .reads import Reads, _unpacked, entry_points


def trace_rows(n, every):
    """nb_hip_ensemble_trace_rows: the records a traced update of n steps makes, 1 + n // every."""
    return int(hip_lib().nb_hip_ensemble_trace_rows(int(n), int(every)))


def _packed(members):
    """a list of (N_b, 8) arrays -> (one packed float32 (sum N_b, 8) array, uint32 sizes)"""
    parts = [as_particles(m) for m in members]
    sizes = np.array([p.shape[0] for p in parts], dtype=np.uint32)
    flat = np.concatenate(parts, axis=0) if parts else np.zeros((0, 8), np.float32)
    return np.ascontiguousarray(flat, dtype=np.float32), sizes


def _dt_array(dts, count):
    a = np.ascontiguousarray(dts, dtype=np.float32)
    if a.shape != (count,):
        raise ValueError(f"expected {count} step sizes")
    return a


class SimBatch(Reads):
    """include/nbody_hip.h SimBatch: B independent worlds of the same size, stepped together (nb_hip_batch_*).

    Particles are float32 arrays of shape (B, n, 8), every member already partitioned (mass > 0 first) with
    `mass_len[b]` massive ones.  Member b ends bit-identical to the same particles alone in a SimPipeline pinned to
    launch_shape().

    SimBatch.ragged(total_lens, mass_lens) makes an ensemble whose members differ in size (nb_hip_ragged_create): set_data
    takes and get_data() / potential() return a LIST of per-member arrays, everything else keeps its shape; member b is
    bit-identical to the same particles as the single member of SimBatch(total_lens[b], [mass_lens[b]])."""

    is_ragged = False
    _lib = staticmethod(hip_lib)
    _ENTRY = entry_points("SimBatch")
    _n = property(lambda self: self.total_len)

    def __init__(self, total_len, mass_len):
        m = np.ascontiguousarray(mass_len, dtype=np.uint32)
        if m.ndim != 1:
            raise ValueError("mass_len must be a sequence with one entry per member")
        self.count, self.total_len, self.mass_len = int(m.shape[0]), int(total_len), m.copy()
        self._h = hip_lib().nb_hip_batch_create(self.count, self.total_len, m.ctypes.data_as(C.POINTER(C.c_uint32)))

    @classmethod
    def ragged(cls, total_lens, mass_lens):
        """nb_hip_ragged_create: member b has total_lens[b] particles, mass_lens[b] of them massive."""
        n = np.ascontiguousarray(total_lens, dtype=np.uint32)
        m = np.ascontiguousarray(mass_lens, dtype=np.uint32)
        if n.ndim != 1 or m.shape != n.shape:
            raise ValueError("total_lens and mass_lens must be sequences with one entry per member")
        self = cls.__new__(cls)
        self.is_ragged = True
        self.count, self.total_lens, self.mass_len = int(n.shape[0]), n.copy(), m.copy()
        self.total_len = int(n.max()) if n.size else 0
        self._h = hip_lib().nb_hip_ragged_create(self.count, n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 m.ctypes.data_as(C.POINTER(C.c_uint32)))
        self.offsets = self.layout()[1]
        return self

    def layout(self):
        """nb_hip_ragged_layout: (sizes uint32 (B,), offsets uint64 (B + 1,)) of the packed arrays; also for a uniform ensemble."""
        sizes, offsets = np.empty(self.count, np.uint32), np.empty(self.count + 1, np.uint64)
        hip_lib().nb_hip_ragged_layout(self._h, sizes.ctypes.data_as(C.POINTER(C.c_uint32)), offsets.ctypes.data_as(C.POINTER(C.c_uint64)))
        return sizes, offsets

    def sizes(self):
        return [int(x) for x in self.layout()[0]]

    def close(self):
        if self._h:
            hip_lib().nb_hip_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, particles):
        if self.is_ragged:
            flat, sizes = _packed(particles)
            assert np.array_equal(sizes, self.total_lens)
            hip_lib().nb_hip_batch_set_data(self._h, flat.ctypes.data)
            return
        a = as_ensemble(particles)
        assert a.shape[:2] == (self.count, self.total_len)
        hip_lib().nb_hip_batch_set_data(self._h, a.ctypes.data)

    def get_data(self):
        if self.is_ragged:
            flat = np.empty((int(self.offsets[-1]), 8), dtype=np.float32)
            hip_lib().nb_hip_batch_get_data(self._h, flat.ctypes.data)
            return _unpacked(flat, self.offsets)
        out = np.empty((self.count, self.total_len, 8), dtype=np.float32)
        hip_lib().nb_hip_batch_get_data(self._h, out.ctypes.data)
        return out

    def get_member(self, b):
        n = int(self.total_lens[b]) if self.is_ragged and 0 <= int(b) < self.count else self.total_len
        out = np.empty((n, 8), dtype=np.float32)
        hip_lib().nb_hip_batch_get_member(self._h, int(b), out.ctypes.data)
        return out

    def update(self, n, dt):
        """Blocking n steps of every member; dt: one step size, or one per member."""
        if np.ndim(dt) == 0:
            hip_lib().nb_hip_batch_update(self._h, n, float(dt))
        else:
            hip_lib().nb_hip_batch_update_dts(self._h, n, _dt_array(dt, self.count).ctypes.data_as(C.POINTER(C.c_float)))

    def step_async(self, n, dts):
        hip_lib().nb_hip_batch_step_async(self._h, n, _dt_array(dts, self.count).ctypes.data_as(C.POINTER(C.c_float)))

    def update_leapfrog(self, n, dt):
        """Blocking n kick-drift-kick steps of every member (include/nbody_leapfrog.h); dt: one step size, or one per member."""
        if np.ndim(dt) == 0:
            hip_lib().nb_hip_ensemble_leapfrog(self._h, n, float(dt))
        else:
            hip_lib().nb_hip_ensemble_leapfrog_dts(self._h, n, _dt_array(dt, self.count).ctypes.data_as(C.POINTER(C.c_float)))

    def last_leapfrog_info(self):
        """Tuning hook: (force launches of the last leapfrog call, whether it primed)."""
        k, primed = C.c_uint32(0), C.c_int(0)
        hip_lib().nb_hip_ensemble_last_leapfrog_info(self._h, C.byref(k), C.byref(primed))
        return int(k.value), bool(primed.value)

    def update_adaptive(self, n, eta, dt_max, dt_min=0.0, span=float("inf"), prime=False, resume=False, leapfrog=False):
        """nb_hip_ensemble_adaptive_steps: n steps, every member with its own step size at every step, chosen on the device.
        Returns (dt_log float32 (n, B), list of B result dicts)."""
        cfg, res = adaptive_cfg(eta, dt_max, dt_min, span, prime, resume=resume, leapfrog=leapfrog), (NbAdaptiveResult * self.count)()
        log = np.zeros((n, self.count), dtype=np.float32)
        hip_lib().nb_hip_ensemble_adaptive_steps(self._h, n, C.byref(cfg), log.ctypes.data, C.byref(res))
        return log, [r.as_dict() for r in res]

    def sync(self):
        hip_lib().nb_hip_batch_sync(self._h)

    def last_ms(self):
        """device ms of the kernels of the last update"""
        return float(hip_lib().nb_hip_batch_last_ms(self._h))

    def dt_uploads(self):
        return int(hip_lib().nb_hip_batch_dt_uploads(self._h))

    def trace(self, n, dt, every):
        """nb_hip_ensemble_trace(_dts): update(n, dt) that records every member's energy on entry and after every `every`-th
        step, in one call.  float64 (R, count, 8) in WorldEnergy field order, R = 1 + n // every; energy_row(a[r, b]) is
        what energy() gives member b for that state."""
        out = np.empty((trace_rows(n, every), self.count, 8), dtype=np.float64)
        if np.ndim(dt) == 0:
            hip_lib().nb_hip_ensemble_trace(self._h, n, float(dt), every, out.ctypes.data)
        else:
            hip_lib().nb_hip_ensemble_trace_dts(self._h, n, _dt_array(dt, self.count).ctypes.data_as(C.POINTER(C.c_float)), every,
                                             out.ctypes.data)
        return out

    def trace_mode(self, mode):
        """tuning hook: 0 = auto, 1 = interleave the diagnostics launches even where the chain records by itself."""
        hip_lib().nb_hip_ensemble_trace_mode(self._h, int(mode))

    def last_trace_info(self):
        """tuning hook: {"fused": 0 / 1, "launches": kernel launches} of the last trace()."""
        fused, launches = C.c_int(0), C.c_uint32(0)
        hip_lib().nb_hip_ensemble_last_trace_info(self._h, C.byref(fused), C.byref(launches))
        return {"fused": fused.value, "launches": launches.value}

    def last_diag_ms(self):
        """tuning hook: device ms of the kernels of the last energy() / potential() / potential_at() / potential_map() /
        acceleration_at() / acceleration_map() / tidal_at() / tidal_map() / profile() / pair_counts() / neighbours() / groups(); 0.0 after a
        call that had nothing to launch."""
        return float(hip_lib().nb_hip_ensemble_last_diag_ms(self._h))

    def render_mode(self, mode):
        """tuning hook: 0 = auto, 1 = the global path (clear, splat, disc pass, shade) also where the tile path applies."""
        hip_lib().nb_hip_ensemble_render_mode(self._h, int(mode))

    def last_render_info(self):
        """tuning hook: {"tile_path": 0 / 1, "launches": launches enqueued} of the last render_counts() / render()."""
        tile, launches = C.c_int(0), C.c_uint32(0)
        hip_lib().nb_hip_ensemble_last_render_info(self._h, C.byref(tile), C.byref(launches))
        return {"tile_path": tile.value, "launches": launches.value}

    def last_render_ms(self):
        """tuning hook: device ms of the kernels of the last bounds() / render_counts() / render()."""
        return float(hip_lib().nb_hip_ensemble_last_render_ms(self._h))

    def launch_shape(self):
        """path "chain" / "lanes" plus the knobs that pin a SimPipeline to the same summation order (pinned_knobs); ragged:
        {"groups": [one such dict per launch group, with its member count], "members": [(group, k, w, lanes) per member]}."""
        path, k, w, lanes, g = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_uint32()
        if self.is_ragged:
            groups, i, total = [], 0, 1
            members = C.c_uint32()
            while i < total:
                total = int(hip_lib().nb_hip_ragged_launch_shape(self._h, i, C.byref(path), C.byref(k), C.byref(w), C.byref(lanes),
                                                                 C.byref(members), C.byref(g)))
                groups.append({"path": "lanes" if path.value else "chain", "k": k.value, "w": w.value, "lanes": lanes.value,
                               "members": members.value, "workgroups": g.value})
                i += 1
            per = []
            grp = C.c_uint32()
            for b in range(self.count):
                hip_lib().nb_hip_ragged_member_shape(self._h, b, C.byref(grp), C.byref(k), C.byref(w), C.byref(lanes))
                per.append((grp.value, k.value, w.value, lanes.value))
            return {"groups": groups, "members": per}
        hip_lib().nb_hip_batch_launch_shape(self._h, C.byref(path), C.byref(k), C.byref(w), C.byref(lanes), C.byref(g))
        return {"path": "lanes" if path.value else "chain", "k": k.value, "w": w.value, "lanes": lanes.value,
                "workgroups": g.value}

    def pinned_knobs(self):
        """SimPipeline.configure(**pinned_knobs()) pins a single pipeline to this ensemble's launch shape."""
        s = self.launch_shape()
        if s["path"] == "chain":
            return dict(k=s["k"], w=s["w"], split=1, unit=8, fused_chain=0)
        return dict(lanes=s["lanes"], w=s["w"], fused_chain=0)
