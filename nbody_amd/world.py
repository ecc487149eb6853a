"""World and WorldBatch: include/nbody.h and include/nbody_batch.h, bound 1:1."""
import ctypes as C

import numpy as np

from ._abi import (PUBLIC_KNOBS, UNIQUE_ID_BYTES, NbAdaptiveResult, RenderView, adaptive_cfg, as_ensemble, as_particles, hip_lib,
                   nbody_lib)
from .batch import _dt_array, _packed, trace_rows
from .reads import Reads, entry_points


class World(Reads):
    """include/nbody.h World, bound 1:1 (CreateWorld / UpdateWorld_CPU / UpdateWorld_GPU / ...)."""

    _lib = staticmethod(nbody_lib)
    _ENTRY = entry_points("World")
    _WORLD_LAYER = True
    _n = property(lambda self: self.size)

    def __init__(self, particles, rank=None, nranks=1, unique_id=None):
        """rank / nranks / unique_id: CreateWorldSharded (extension), one World per process and GPU."""
        a = as_particles(particles)
        self.size = a.shape[0]
        if rank is None:
            self._h = nbody_lib().CreateWorld(a.ctypes.data, self.size)
        else:
            idbuf = (C.c_ubyte * UNIQUE_ID_BYTES).from_buffer_copy(unique_id) if unique_id is not None else None
            self._h = nbody_lib().CreateWorldSharded(a.ctypes.data, self.size, rank, nranks, idbuf)

    def close(self):
        if self._h:
            nbody_lib().DestroyWorld(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def particles(self):
        n = C.c_uint32(0)
        p = nbody_lib().GetWorldParticles(self._h, C.byref(n))
        if n.value == 0:
            return np.empty((0, 8), dtype=np.float32)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value, 8)).copy()

    def pipeline(self):
        """GetWorldPipeline: the SimPipeline handle behind this World (for nb_hip_configure / the tuning hooks)."""
        return nbody_lib().GetWorldPipeline(self._h)

    def tune(self, **knobs):
        """Set knobs on the World's pipeline (nb_hip_configure for the public five, nb_hip_tune for the hooks); returns the
        previous value of each, so that a caller can see that a knob took."""
        old = {}
        for k, v in knobs.items():
            fn = hip_lib().nb_hip_configure if k in PUBLIC_KNOBS else hip_lib().nb_hip_tune
            old[k] = int(fn(self.pipeline(), k.encode(), int(v)))
        return old

    def update_cpu(self, dt, n):
        nbody_lib().UpdateWorld_CPU(self._h, dt, n)

    def update_gpu(self, dt, n):
        nbody_lib().UpdateWorld_GPU(self._h, dt, n)

    def _adaptive(self, fn, n, cfg):
        res, log = NbAdaptiveResult(), np.zeros(n, dtype=np.float32)
        fn(self._h, n, C.byref(cfg), log.ctypes.data, C.byref(res))
        return log, res.as_dict()

    def update_gpu_leapfrog(self, dt, n):
        """UpdateWorld_GPU_Leapfrog (include/nbody_leapfrog.h): n kick-drift-kick steps of size dt on the device."""
        nbody_lib().UpdateWorld_GPU_Leapfrog(self._h, dt, n)

    def update_cpu_leapfrog(self, dt, n):
        """UpdateWorld_CPU_Leapfrog: the same on the host cores."""
        nbody_lib().UpdateWorld_CPU_Leapfrog(self._h, dt, n)

    def update_gpu_adaptive(self, n, eta, dt_max, dt_min=0.0, span=float("inf"), prime=False, leapfrog=False):
        """UpdateWorld_GPU_Adaptive (include/nbody_adaptive.h): (dt_log float32 (n,), result dict)."""
        return self._adaptive(nbody_lib().UpdateWorld_GPU_Adaptive, n, adaptive_cfg(eta, dt_max, dt_min, span, prime, leapfrog=leapfrog))

    def update_cpu_adaptive(self, n, eta, dt_max, dt_min=0.0, span=float("inf"), prime=False, leapfrog=False):
        """UpdateWorld_CPU_Adaptive: the same on the host cores."""
        return self._adaptive(nbody_lib().UpdateWorld_CPU_Adaptive, n, adaptive_cfg(eta, dt_max, dt_min, span, prime, leapfrog=leapfrog))

    def timestep(self, eta, dt_max, dt_min=0.0):
        """GetWorldTimestep: the criterion alone (no span clip) for the newest state; changes nothing."""
        cfg, dt = adaptive_cfg(eta, dt_max, dt_min), C.c_float(0.0)
        nbody_lib().GetWorldTimestep(self._h, C.byref(cfg), C.byref(dt))
        return float(dt.value)

    def advance_gpu(self, span, eta, dt_max, dt_min=0.0, prime=False, chunk=0, max_steps=4096, leapfrog=False):
        """AdvanceWorld_GPU: adaptive calls until `span` is covered (or max_steps steps are made); (dt_log float32 of the
        steps made, idle ones included, result dict)."""
        cfg, res = adaptive_cfg(eta, dt_max, dt_min, prime=prime, chunk=chunk, leapfrog=leapfrog), NbAdaptiveResult()
        log = np.zeros(max_steps, dtype=np.float32)
        nbody_lib().AdvanceWorld_GPU(self._h, float(span), C.byref(cfg), max_steps, log.ctypes.data, C.byref(res))
        return log[:res.steps + res.idle_steps].copy(), res.as_dict()

    def fit_view(self, width, height):
        """FitWorldView: the RenderView that shows every finite particle on a width x height screen."""
        v = RenderView()
        nbody_lib().FitWorldView(self._h, width, height, C.byref(v))
        return v


class WorldBatch(Reads):
    """include/nbody_batch.h WorldBatch, bound 1:1: (B, n, 8) particles in caller order; every member is partitioned
    like CreateWorld partitions it.  WorldBatch.ragged(list of (N_b, 8) arrays) makes a batch whose members differ in size
    (include/nbody_batch_ragged.h): particles() and potential() then return lists of per-member arrays."""

    is_ragged = False
    _lib = staticmethod(nbody_lib)
    _ENTRY = entry_points("WorldBatch")
    _WORLD_LAYER = True
    _n = property(lambda self: self.size)

    def __init__(self, particles):
        a = as_ensemble(particles)
        self.count, self.size = int(a.shape[0]), int(a.shape[1])
        self._h = nbody_lib().CreateWorldBatch(a.ctypes.data, self.size, self.count)

    @classmethod
    def ragged(cls, members):
        flat, sizes = _packed(members)
        self = cls.__new__(cls)
        self.is_ragged = True
        self.count, self._sizes = int(sizes.shape[0]), sizes
        self.size = int(sizes.max()) if sizes.size else 0
        self.offsets = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
        self._h = nbody_lib().CreateWorldBatchRagged(flat.ctypes.data, sizes.ctypes.data_as(C.POINTER(C.c_uint32)), self.count)
        return self

    def sizes(self):
        return [int(x) for x in self._sizes] if self.is_ragged else [self.size] * self.count

    def close(self):
        if self._h:
            nbody_lib().DestroyWorldBatch(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def member(self, b):
        n = C.c_uint32(0)
        p = nbody_lib().GetWorldBatchParticles(self._h, int(b), C.byref(n))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value, 8)).copy()

    def particles(self):
        if self.is_ragged:
            return [self.member(b) for b in range(self.count)]
        return np.stack([self.member(b) for b in range(self.count)])

    def update_gpu(self, dt, n):
        if np.ndim(dt) == 0:
            nbody_lib().UpdateWorldBatch_GPU(self._h, float(dt), n)
        else:
            nbody_lib().UpdateWorldBatch_GPU_dts(self._h, _dt_array(dt, self.count).ctypes.data_as(C.POINTER(C.c_float)), n)

    def update_gpu_leapfrog(self, dt, n):
        """UpdateWorldBatch_GPU_Leapfrog(_dts) (include/nbody_leapfrog.h); dt: one step size, or one per member."""
        if np.ndim(dt) == 0:
            nbody_lib().UpdateWorldBatch_GPU_Leapfrog(self._h, float(dt), n)
        else:
            nbody_lib().UpdateWorldBatch_GPU_Leapfrog_dts(self._h, _dt_array(dt, self.count).ctypes.data_as(C.POINTER(C.c_float)), n)

    def update_gpu_adaptive(self, n, eta, dt_max, dt_min=0.0, span=float("inf"), prime=False, leapfrog=False):
        """UpdateWorldBatch_GPU_Adaptive (include/nbody_adaptive.h): (dt_log float32 (n, B), list of B result dicts)."""
        cfg, res = adaptive_cfg(eta, dt_max, dt_min, span, prime, leapfrog=leapfrog), (NbAdaptiveResult * self.count)()
        log = np.zeros((n, self.count), dtype=np.float32)
        nbody_lib().UpdateWorldBatch_GPU_Adaptive(self._h, n, C.byref(cfg), log.ctypes.data, C.byref(res))
        return log, [r.as_dict() for r in res]

    def advance_gpu(self, span, eta, dt_max, dt_min=0.0, prime=False, chunk=0, max_steps=4096, leapfrog=False):
        """AdvanceWorldBatch_GPU: every member covers `span` (or max_steps steps are made); (dt_log float32 (steps made, B)
        with the idle steps of members that finished early, list of B result dicts)."""
        cfg, res = adaptive_cfg(eta, dt_max, dt_min, prime=prime, chunk=chunk, leapfrog=leapfrog), (NbAdaptiveResult * self.count)()
        log = np.zeros((max_steps, self.count), dtype=np.float32)
        nbody_lib().AdvanceWorldBatch_GPU(self._h, float(span), C.byref(cfg), max_steps, log.ctypes.data, C.byref(res))
        made = max((r.steps + r.idle_steps for r in res), default=0)
        return log[:made].copy(), [r.as_dict() for r in res]

    def update_gpu_traced(self, dt, n, every):
        """UpdateWorldBatch_GPU_Traced(_dts): update_gpu(dt, n) that records every member's energy on entry and after every
        `every`-th step; float64 (R, count, 8) like SimBatch.trace."""
        out = np.empty((trace_rows(n, every), self.count, 8), dtype=np.float64)
        if np.ndim(dt) == 0:
            nbody_lib().UpdateWorldBatch_GPU_Traced(self._h, float(dt), n, every, out.ctypes.data)
        else:
            nbody_lib().UpdateWorldBatch_GPU_Traced_dts(self._h, _dt_array(dt, self.count).ctypes.data_as(C.POINTER(C.c_float)), n,
                                                        every, out.ctypes.data)
        return out

    def fit_views(self, width, height):
        """FitWorldBatchViews: a list of B RenderViews, each showing every finite particle of its member."""
        arr = (RenderView * self.count)()
        nbody_lib().FitWorldBatchViews(self._h, width, height, arr)
        return [RenderView.from_buffer_copy(v) for v in arr]
