"""SimPipeline, the inner seam of include/nbody_hip.h as an object, and LocalShardGroup."""
import ctypes as C
import os

import numpy as np

from ._abi import (ALLGATHER_FN, PUBLIC_KNOBS, UNIQUE_ID_BYTES, NbAdaptiveResult, WorldData, adaptive_cfg, as_particles, hip_lib)
from .reads import Reads, entry_points


class SimPipeline(Reads):
    """The inner seam (reference src/lib/sim_gpu.h:21-36) as an object.

    `particles` passed to set_data must already be partitioned (mass > 0 first) with
    `mass_len` massive ones, exactly what reference src/lib/world.c:32-58 hands its backend.
    """

    _lib = staticmethod(hip_lib)
    _ENTRY = entry_points("SimPipeline")
    _n = property(lambda self: self.total_len)

    def __init__(self, total_len, mass_len, rank=0, nranks=1, unique_id=None, allgather=None, direct=False):
        """allgather: a Python callable (buf: writable uint8 array of shape (nranks, bytes_per_rank), rank, nranks) that
        fills every row with its owner's bytes -- the caller-supplied host transport (CreateSimPipelineShardedWith);
        direct=True: the same callable carries only IPC handles and step barriers, the data goes device to device
        (CreateSimPipelineShardedDirect)."""
        L = hip_lib()
        wd = WorldData(total_len, mass_len, 0.0)
        self._cb = None
        if allgather is not None:
            def thunk(_ctx, buf, bytes_per_rank, r, n):
                # An exception must not escape into ctypes (it would be printed and swallowed, the staging buffer would
                # keep stale peer slots, and this rank would step on them while the others block in their next
                # collective).  The process has touched the GPU: report and leave with a fresh exit, no retry.
                try:
                    rows = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), shape=(n, int(bytes_per_rank)))
                    allgather(rows, r, n)
                except BaseException:
                    import sys
                    import traceback
                    traceback.print_exc()
                    print(f"[nbody_amd] rank {r} of {n}: the caller-supplied all-gather raised; exiting (5)", file=sys.stderr,
                          flush=True)
                    os._exit(5)
            self._cb = ALLGATHER_FN(thunk)   # must outlive the pipeline
            create = L.CreateSimPipelineShardedDirect if direct else L.CreateSimPipelineShardedWith
            self._h = create(wd, rank, nranks, self._cb, None)
        elif nranks > 1 or unique_id is not None:
            idbuf = (C.c_ubyte * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
            self._h = L.CreateSimPipelineSharded(wd, rank, nranks, idbuf)
        else:
            self._h = L.CreateSimPipeline(wd)
        self.total_len, self.mass_len = total_len, mass_len
        self.rank, self.nranks = rank, nranks
        self.configure(timing=1)   # tooling wants last_step_ms(); the C default is off (it costs a frame loop 3-7 us)

    def close(self):
        if self._h:
            hip_lib().DestroySimPipeline(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, particles):
        a = as_particles(particles)
        assert a.shape[0] == self.total_len
        hip_lib().SetSimulationData(self._h, a.ctypes.data)

    def get_data(self):
        out = np.empty((self.total_len, 8), dtype=np.float32)
        hip_lib().GetSimulationData(self._h, out.ctypes.data)
        return out

    def update(self, n, dt):
        """Blocking n steps (PerformSimUpdate)."""
        hip_lib().PerformSimUpdate(self._h, n, dt)

    def step_async(self, n, dt):
        hip_lib().nb_hip_step_async(self._h, n, dt)

    def update_leapfrog(self, n, dt):
        """nb_hip_leapfrog_steps: blocking n kick-drift-kick steps of size dt (include/nbody_leapfrog.h)."""
        hip_lib().nb_hip_leapfrog_steps(self._h, n, dt)

    def update_leapfrog_async(self, n, dt):
        """nb_hip_leapfrog_steps_async: enqueue only; sync() waits."""
        hip_lib().nb_hip_leapfrog_steps_async(self._h, n, dt)

    def last_leapfrog_info(self):
        """Tuning hook: (force launches of the last leapfrog call, whether it primed)."""
        k, primed = C.c_uint32(0), C.c_int(0)
        hip_lib().nb_hip_last_leapfrog_info(self._h, C.byref(k), C.byref(primed))
        return int(k.value), bool(primed.value)

    def update_adaptive(self, n, eta, dt_max, dt_min=0.0, span=float("inf"), prime=False, resume=False, leapfrog=False):
        """nb_hip_adaptive_steps: n steps, each of the size the criterion of include/nbody_adaptive.h gives for the state
        before it, chosen on the device.  Returns (dt_log float32 (n,), result dict)."""
        cfg, res, log = adaptive_cfg(eta, dt_max, dt_min, span, prime, resume=resume, leapfrog=leapfrog), NbAdaptiveResult(), np.zeros(n, dtype=np.float32)
        hip_lib().nb_hip_adaptive_steps(self._h, n, C.byref(cfg), log.ctypes.data, C.byref(res))
        return log, res.as_dict()

    def update_adaptive_async(self, n, eta, dt_max, dt_min=0.0, span=float("inf"), prime=False, resume=False, leapfrog=False):
        """nb_hip_adaptive_steps_async: enqueue only; adaptive_collect(n) fetches the log and the result."""
        cfg = adaptive_cfg(eta, dt_max, dt_min, span, prime, resume=resume, leapfrog=leapfrog)
        hip_lib().nb_hip_adaptive_steps_async(self._h, n, C.byref(cfg))

    def adaptive_collect(self, n):
        res, log = NbAdaptiveResult(), np.zeros(n, dtype=np.float32)
        hip_lib().nb_hip_adaptive_collect(self._h, log.ctypes.data, C.byref(res))
        return log, res.as_dict()

    def timestep(self, eta, dt_max, dt_min=0.0):
        """nb_hip_timestep: the criterion alone for the latest state (no span clip); changes nothing."""
        cfg, dt = adaptive_cfg(eta, dt_max, dt_min), C.c_float(0.0)
        hip_lib().nb_hip_timestep(self._h, C.byref(cfg), C.byref(dt))
        return float(dt.value)

    def sync(self):
        hip_lib().nb_hip_sync(self._h)

    def last_step_ms(self):
        launches = C.c_uint32(0)
        ms = hip_lib().nb_hip_last_step_ms(self._h, C.byref(launches))
        return float(ms), int(launches.value)

    def finish_launches(self):
        return int(hip_lib().nb_hip_last_finish_launches(self._h))

    def step_breakdown(self):
        """(steps covered, kernel ms, all-gather ms) of the last update of a sharded pipeline."""
        k, c = C.c_double(0.0), C.c_double(0.0)
        steps = hip_lib().nb_hip_last_step_breakdown(self._h, C.byref(k), C.byref(c))
        return int(steps), float(k.value), float(c.value)

    def comm_info(self):
        """What the RCCL communicator itself reports (ncclCommCount etc.); owns_comm False when there is none."""
        n, r, d, v, ms = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
        path = C.create_string_buffer(256)
        own = hip_lib().nb_hip_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d), C.byref(v), C.byref(ms), path, 256)
        return {"owns_comm": bool(own), "nranks": n.value, "rank": r.value, "device": d.value, "rccl_version": v.value,
                "first_gather_ms": ms.value, "rccl_lib": path.value.decode()}

    def comm_bringup(self):
        """nb_hip_comm_bringup: ncclCommInitRank host ms, first all-gather device ms, one warm 8-byte all-gather in device us."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        own = hip_lib().nb_hip_comm_bringup(self._h, C.byref(a), C.byref(b), C.byref(c))
        return {"owns_comm": bool(own), "comm_init_ms": a.value, "first_gather_ms": b.value, "small_gather_us": c.value}

    def graph_stats(self):
        """cached hipGraph chains and how often a new step size was written to device memory."""
        uploads = C.c_uint32(0)
        cached = hip_lib().nb_hip_graph_stats(self._h, C.byref(uploads))
        return {"cached": int(cached), "dt_uploads": int(uploads.value)}

    def last_diag_ms(self):
        """tuning hook: device ms of the kernels of the last energy() / potential() / potential_at() / potential_map() /
        acceleration_at() / acceleration_map() / tidal_at() / tidal_map() / profile() / pair_counts() / neighbours() / groups(); 0.0 after a
        call that had nothing to launch."""
        return float(hip_lib().nb_hip_last_diag_ms(self._h))

    def last_render_ms(self):
        """tuning hook: (device ms of the last render, [bounds, clear + splat, disc, shade]); the last three need
        configure(render_detail=1)."""
        parts = (C.c_double * 4)()
        total = hip_lib().nb_hip_last_render_ms(self._h, parts)
        return float(total), [float(v) for v in parts]

    def fused_steps(self):
        """steps of the last update that ran inside one-workgroup chain launches (knob fused_chain)."""
        return int(hip_lib().nb_hip_last_fused_steps(self._h))

    def last_deal(self):
        """tuning hook: (dealt, items, extra workgroups) of the step launches of the last update (knob deal)."""
        items, extra = C.c_uint32(0), C.c_uint32(0)
        dealt = hip_lib().nb_hip_last_deal(self._h, C.byref(items), C.byref(extra))
        return bool(dealt), int(items.value), int(extra.value)

    def deal_counter(self):
        """tuning hook: the ticket counter of the dealt launches, read back after a sync (0 between launches)."""
        return int(hip_lib().nb_hip_deal_counter(self._h))

    def configure(self, **knobs):
        """The five knobs of include/nbody_hip.h go through nb_hip_configure; anything else is a launch-shape / experiment
        hook of nbody_hip_tuning.h (nb_hip_tune; aborts on an unknown name like the public call does)."""
        for k, v in knobs.items():
            fn = hip_lib().nb_hip_configure if k in PUBLIC_KNOBS else hip_lib().nb_hip_tune
            fn(self._h, k.encode(), int(v))

    def launch_shape(self):
        k, w, v, sp, g = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_uint32()
        hip_lib().nb_hip_launch_shape(self._h, C.byref(k), C.byref(w), C.byref(v), C.byref(sp), C.byref(g))
        return {"k": k.value, "w": w.value, "variant": "smem" if v.value else "lds", "split": sp.value,
                "workgroups": g.value, "unit": int(hip_lib().nb_hip_launch_unit(self._h)),
                "lanes": int(hip_lib().nb_hip_launch_lanes(self._h))}


class LocalShardGroup:
    """nranks shards of one world inside this process (include/nbody_hip.h "Local transport")."""

    def __init__(self, total_len, mass_len, nranks, **knobs):
        L = hip_lib()
        self.nranks = nranks
        self._arr = (C.c_void_p * nranks)()
        L.nb_hip_local_group_create(WorldData(total_len, mass_len, 0.0), nranks, self._arr)
        self.members = []
        for r in range(nranks):
            m = SimPipeline.__new__(SimPipeline)
            m._h = self._arr[r]
            m.total_len, m.mass_len, m.rank, m.nranks = total_len, mass_len, r, nranks
            m.configure(timing=1, **knobs)
            self.members.append(m)

    def set_data(self, particles):
        for m in self.members:
            m.set_data(particles)

    def step(self, n, dt):
        hip_lib().nb_hip_local_group_step(self._arr, self.nranks, n, dt)

    def get_data(self, rank=0):
        return self.members[rank].get_data()

    def close(self):
        for m in self.members:
            m.close()
        self.members = []
