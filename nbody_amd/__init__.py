"""nbody_amd -- Python view of the MI355X-native N-body engine (for tests, bench.py and tooling).

The product is C: `lib/libnbody_hip.so` (HIP kernels + the C-ABI of include/nbody_hip.h) and
`lib/libnbody.so` (the include/nbody.h / galaxy.h surface, C host code).  This module only binds
them with ctypes; no arithmetic happens in Python and there is no fallback: if the libraries are
missing, importing the bound functions raises, and any GPU call without a gfx950 device aborts
inside the library (reference error convention, src/lib/util.h:17-29).

Particles travel as float32 arrays of shape (n, 8): pos.xy vel.xy acc.xy mass radius --
byte-identical to `Particle[n]` (include/nbody.h).
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_DIR = os.path.join(PKG_DIR, "lib")
HIP_SO = os.environ.get("NBODY_HIP_SO") or os.path.join(LIB_DIR, "libnbody_hip.so")  # override: kernel experiments
NBODY_SO = os.path.join(LIB_DIR, "libnbody.so")



def _nb_g_from_header():
    """NB_G as include/nbody.h spells it -- the one place the value is written down."""
    import re
    with open(os.path.join(ROOT, "include", "nbody.h")) as f:
        return float(re.search(r"^#define\s+NB_G\s+([0-9.eE+-]+)f?\s*$", f.read(), re.M).group(1))


NB_G = _nb_g_from_header()
UNIQUE_ID_BYTES = 128
CLOCK_SAMPLER_MAX_MS = 20000.0   # include/nbody_hip.h NB_CLOCK_SAMPLER_MAX_MS: larger bounds are clamped by the library


class WorldData(C.Structure):
    """include/nbody_hip.h WorldData (reference src/lib/sim_gpu.h:8-12)."""
    _fields_ = [("total_len", C.c_uint32), ("mass_len", C.c_uint32), ("dt", C.c_float)]


class WorldEnergy(C.Structure):
    """include/nbody_diag.h WorldEnergy (float64 sums over the massive particles)."""
    _fields_ = [("kinetic", C.c_double), ("potential", C.c_double), ("mass", C.c_double), ("momentum", C.c_double * 2),
                ("angular_momentum", C.c_double), ("center_of_mass", C.c_double * 2)]

    def as_dict(self):
        return {"kinetic": self.kinetic, "potential": self.potential, "total": self.kinetic + self.potential,
                "mass": self.mass, "momentum": (self.momentum[0], self.momentum[1]),
                "angular_momentum": self.angular_momentum,
                "center_of_mass": (self.center_of_mass[0], self.center_of_mass[1])}


def energy_row(row):
    """One [8] row of a traced update (WorldEnergy field order: kinetic, potential, mass, momentum x / y, angular momentum,
    centre of mass x / y) as the dict energy() returns for that state: rows compare with `==`."""
    e = WorldEnergy()
    C.memmove(C.byref(e), np.ascontiguousarray(row, dtype=np.float64).ctypes.data, C.sizeof(WorldEnergy))
    return e.as_dict()


def trace_rows(n, every):
    """nb_hip_ensemble_trace_rows: the records a traced update of n steps makes, 1 + n // every."""
    return int(hip_lib().nb_hip_ensemble_trace_rows(int(n), int(every)))


class RenderView(C.Structure):
    """include/nbody_render.h RenderView: sx = (x - target) * zoom + offset on a width x height screen."""
    _fields_ = [("target", C.c_float * 2), ("offset", C.c_float * 2), ("zoom", C.c_float), ("width", C.c_uint32),
                ("height", C.c_uint32), ("core_mass", C.c_float)]

    @classmethod
    def make(cls, target, offset, zoom, width, height, core_mass):
        return cls((C.c_float * 2)(*target), (C.c_float * 2)(*offset), zoom, width, height, core_mass)

    def as_dict(self):
        return {"target": (self.target[0], self.target[1]), "offset": (self.offset[0], self.offset[1]), "zoom": self.zoom,
                "width": self.width, "height": self.height, "core_mass": self.core_mass}


class RenderPalette(C.Structure):
    """include/nbody_render.h RenderPalette: RGBA background, RGBA per class, the count at which a pixel saturates."""
    _fields_ = [("background", C.c_uint8 * 4), ("color", (C.c_uint8 * 4) * 3), ("saturation", C.c_uint32)]

    @classmethod
    def make(cls, background, color, saturation):
        return cls((C.c_uint8 * 4)(*background), ((C.c_uint8 * 4) * 3)(*[(C.c_uint8 * 4)(*c) for c in color]), saturation)


def default_palette():
    """DefaultRenderPalette (include/nbody_render.h)."""
    p = RenderPalette()
    nbody_lib().DefaultRenderPalette(C.byref(p))
    return p


class NbAdaptive(C.Structure):
    """include/nbody_adaptive.h NbAdaptive: the configuration of adaptive steps."""
    _fields_ = [("eta", C.c_float), ("dt_min", C.c_float), ("dt_max", C.c_float), ("flags", C.c_uint32), ("span", C.c_double),
                ("chunk", C.c_uint32), ("reserved", C.c_uint32)]


class NbAdaptiveResult(C.Structure):
    """include/nbody_adaptive.h NbAdaptiveResult."""
    _fields_ = [("elapsed", C.c_double), ("steps", C.c_uint32), ("idle_steps", C.c_uint32), ("dt_last", C.c_float),
                ("dt_smallest", C.c_float)]

    def as_dict(self):
        return {"elapsed": self.elapsed, "steps": int(self.steps), "idle_steps": int(self.idle_steps), "dt_last": self.dt_last,
                "dt_smallest": self.dt_smallest}


NB_ADAPT_PRIME = 1      # include/nbody_adaptive.h
NB_ADAPT_CONTINUE = 2
NB_ADAPT_LEAPFROG = 4   # every step a kick-drift-kick step (include/nbody_leapfrog.h)


def adaptive_cfg(eta, dt_max, dt_min=0.0, span=float("inf"), prime=False, chunk=0, resume=False, leapfrog=False):
    """NbAdaptive from the keyword arguments the adaptive methods share; eta and dt_max have no default."""
    flags = (NB_ADAPT_PRIME if prime else 0) | (NB_ADAPT_CONTINUE if resume else 0) | (NB_ADAPT_LEAPFROG if leapfrog else 0)
    return NbAdaptive(float(eta), float(dt_min), float(dt_max), flags, float(span), int(chunk), 0)


NB_PROFILE_BY_MASS = 0     # include/nbody_profile.h
NB_PROFILE_BY_NUMBER = 1
NB_PROFILE_MAX_BINS = 254
NB_PROFILE_QTY = 6
NB_PROFILE_CHUNK = 1024


class WorldProfileSpec(C.Structure):
    """include/nbody_profile.h WorldProfileSpec; `edges` points into an array the caller keeps alive."""
    _fields_ = [("edges", C.c_void_p), ("bins", C.c_uint32), ("centre", C.c_float * 2), ("centre_velocity", C.c_float * 2),
                ("weights", C.c_int)]


NB_PAIRS_MM, NB_PAIRS_MT, NB_PAIRS_TT, NB_PAIRS_ALL = 1, 2, 4, 7     # include/nbody_paircount.h
NB_PAIRS_MAX_BINS = 254
NB_PAIRS_COLUMNS = 3
NB_PAIRS_TABLE = 255     # nbody_amd/csrc/paircount_common.h


class WorldPairSpec(C.Structure):
    """include/nbody_paircount.h WorldPairSpec; `edges` points into an array the caller keeps alive."""
    _fields_ = [("edges", C.c_void_p), ("bins", C.c_uint32), ("classes", C.c_uint32)]


NB_NEIGH_MASSIVE, NB_NEIGH_MASSLESS, NB_NEIGH_ALL = 1, 2, 3     # include/nbody_neighbour.h
NB_NEIGH_NONE = 0xFFFFFFFF


class WorldNeighbourSpec(C.Structure):
    """include/nbody_neighbour.h WorldNeighbourSpec."""
    _fields_ = [("receivers", C.c_uint32), ("sources", C.c_uint32), ("radius", C.c_float)]


class NbShardPlan(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("mass_chunk", "zero_chunk", "mass_begin", "mass_count",
                                          "zero_begin", "zero_count", "src_padded")]


# include/nbody_hip.h NbAllGatherFn: (ctx, buf, bytes_per_rank, rank, nranks)
ALLGATHER_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int)

# every symbol include/nbody_hip.h declares: (restype, argtypes)
HIP_API = {
    "CreateSimPipeline": (C.c_void_p, [WorldData]),
    "DestroySimPipeline": (None, [C.c_void_p]),
    "GetSimulationData": (None, [C.c_void_p, C.c_void_p]),
    "SetSimulationData": (None, [C.c_void_p, C.c_void_p]),
    "PerformSimUpdate": (None, [C.c_void_p, C.c_uint32, C.c_float]),
    "nb_hip_device_count": (C.c_int, []),
    "nb_hip_set_device": (None, [C.c_int]),
    "nb_hip_device_info": (None, [C.c_char_p, C.c_uint32]),
    "nb_hip_step_async": (None, [C.c_void_p, C.c_uint32, C.c_float]),
    "nb_hip_sync": (None, [C.c_void_p]),
    "nb_hip_last_step_ms": (C.c_double, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "nb_hip_last_finish_launches": (C.c_uint32, [C.c_void_p]),
    "nb_hip_last_step_breakdown": (C.c_uint32, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "nb_hip_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_char_p, C.c_uint32]),
    "nb_hip_comm_bringup": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "nb_hip_preflight_peers": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "nb_hip_preflight_ipc_export": (C.c_int, [C.c_void_p, C.c_uint32]),
    "nb_hip_preflight_ipc_open": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]),
    "nb_hip_preflight_ipc_release": (None, []),
    "nb_hip_error_string": (C.c_char_p, [C.c_int]),
    "nb_hip_graph_stats": (C.c_uint32, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "nb_hip_runtime_version": (C.c_int, []),
    "nb_hip_probe_clock": (C.c_int, [C.c_double] + [C.POINTER(C.c_double)] * 5),
    "nb_hip_clock_sampler_begin": (C.c_int, [C.c_double, C.c_double]),
    "nb_hip_clock_sampler_end": (C.c_int, [C.POINTER(C.c_double)] * 6 + [C.POINTER(C.c_uint32)]),
    "nb_hip_note_host_array": (None, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "nb_hip_configure": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "nb_hip_launch_shape": (None, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "nb_hip_plan_launch": (None, [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "nb_hip_comm_unique_id": (None, [C.c_void_p]),
    "CreateSimPipelineSharded": (C.c_void_p, [WorldData, C.c_int, C.c_int, C.c_void_p]),
    "CreateSimPipelineShardedWith": (C.c_void_p, [WorldData, C.c_int, C.c_int, ALLGATHER_FN, C.c_void_p]),
    "CreateSimPipelineShardedDirect": (C.c_void_p, [WorldData, C.c_int, C.c_int, ALLGATHER_FN, C.c_void_p]),
    "nb_hip_shard_plan": (NbShardPlan, [C.c_uint32, C.c_uint32, C.c_int, C.c_int]),
    "nb_hip_local_group_create": (C.c_int, [WorldData, C.c_int, C.POINTER(C.c_void_p)]),
    "nb_hip_local_group_step": (None, [C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_float]),
    "nb_hip_energy": (None, [C.c_void_p, C.POINTER(WorldEnergy)]),
    "nb_hip_potential": (None, [C.c_void_p, C.c_void_p]),
    "nb_hip_bounds": (None, [C.c_void_p, C.c_void_p]),
    "nb_hip_render_counts": (None, [C.c_void_p, C.POINTER(RenderView), C.c_void_p]),
    "nb_hip_render_rgba": (None, [C.c_void_p, C.POINTER(RenderView), C.POINTER(RenderPalette), C.c_void_p]),
    "nb_hip_potential_at": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "nb_hip_potential_map": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    "nb_hip_acceleration_at": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "nb_hip_acceleration_map": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    "nb_hip_tidal_at": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "nb_hip_tidal_map": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    "nb_hip_profile": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nb_hip_ensemble_profile": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nb_hip_pair_counts": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "nb_hip_ensemble_pair_counts": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "nb_hip_neighbours": (None, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nb_hip_ensemble_neighbours": (None, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nb_hip_batch_create": (C.c_void_p, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "nb_hip_batch_destroy": (None, [C.c_void_p]),
    "nb_hip_batch_set_data": (None, [C.c_void_p, C.c_void_p]),
    "nb_hip_batch_get_data": (None, [C.c_void_p, C.c_void_p]),
    "nb_hip_batch_get_member": (None, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "nb_hip_batch_update": (None, [C.c_void_p, C.c_uint32, C.c_float]),
    "nb_hip_batch_update_dts": (None, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]),
    "nb_hip_batch_step_async": (None, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]),
    "nb_hip_batch_sync": (None, [C.c_void_p]),
    "nb_hip_batch_last_ms": (C.c_double, [C.c_void_p]),
    "nb_hip_batch_dt_uploads": (C.c_uint32, [C.c_void_p]),
    "nb_hip_batch_launch_shape": (None, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "nb_hip_ensemble_energy": (None, [C.c_void_p, C.POINTER(WorldEnergy)]),
    "nb_hip_ensemble_potential": (None, [C.c_void_p, C.c_void_p]),
    "nb_hip_ensemble_trace_rows": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "nb_hip_ensemble_trace": (None, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]),
    "nb_hip_ensemble_trace_dts": (None, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.c_uint32, C.c_void_p]),
    "nb_hip_ensemble_bounds": (None, [C.c_void_p, C.c_void_p]),
    "nb_hip_ensemble_render_counts": (None, [C.c_void_p, C.POINTER(RenderView), C.c_void_p]),
    "nb_hip_ensemble_render_rgba": (None, [C.c_void_p, C.POINTER(RenderView), C.POINTER(RenderPalette), C.c_void_p]),
    "nb_hip_ragged_create": (C.c_void_p, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "nb_hip_ragged_layout": (None, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "nb_hip_ragged_launch_shape": (C.c_uint32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "nb_hip_ragged_member_shape": (None, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int)]),
    "nb_hip_ensemble_potential_at": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "nb_hip_ensemble_potential_map": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    "nb_hip_ensemble_acceleration_at": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "nb_hip_ensemble_acceleration_map": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    "nb_hip_ensemble_tidal_at": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "nb_hip_ensemble_tidal_map": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    "nb_hip_adaptive_steps": (None, [C.c_void_p, C.c_uint32, C.POINTER(NbAdaptive), C.c_void_p, C.POINTER(NbAdaptiveResult)]),
    "nb_hip_adaptive_steps_async": (None, [C.c_void_p, C.c_uint32, C.POINTER(NbAdaptive)]),
    "nb_hip_adaptive_collect": (None, [C.c_void_p, C.c_void_p, C.POINTER(NbAdaptiveResult)]),
    "nb_hip_timestep": (None, [C.c_void_p, C.POINTER(NbAdaptive), C.POINTER(C.c_float)]),
    "nb_hip_ensemble_adaptive_steps": (None, [C.c_void_p, C.c_uint32, C.POINTER(NbAdaptive), C.c_void_p, C.c_void_p]),
    "nb_hip_leapfrog_steps": (None, [C.c_void_p, C.c_uint32, C.c_float]),
    "nb_hip_leapfrog_steps_async": (None, [C.c_void_p, C.c_uint32, C.c_float]),
    "nb_hip_ensemble_leapfrog": (None, [C.c_void_p, C.c_uint32, C.c_float]),
    "nb_hip_ensemble_leapfrog_dts": (None, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]),
    "nb_hip_version": (C.c_int, []),
}

# nbody_amd/csrc/nbody_hip_tuning.h: test and tooling hooks, exported by the library but NOT part of the C-ABI
TUNE_API = {
    "nb_hip_tune": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "nb_hip_tuning_build": (C.c_int, []),
    "nb_hip_launch_unit": (C.c_int, [C.c_void_p]),
    "nb_hip_last_fused_steps": (C.c_uint32, [C.c_void_p]),
    "nb_hip_launch_lanes": (C.c_int, [C.c_void_p]),
    "nb_hip_plan_launch_unit": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int]),
    "nb_hip_plan_fused_finish": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int]),
    "nb_hip_last_deal": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "nb_hip_plan_deal": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int]),
    "nb_hip_deal_item": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "nb_hip_deal_counter": (C.c_uint32, [C.c_void_p]),
    "nb_hip_plan_launch_lanes": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]),
    "nb_hip_last_diag_ms": (C.c_double, [C.c_void_p]),
    "nb_hip_pair_thresholds": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "nb_hip_neighbour_span": (C.c_uint32, [C.c_uint32]),
    "nb_hip_last_render_ms": (C.c_double, [C.c_void_p, C.POINTER(C.c_double)]),
    "nb_hip_ensemble_last_diag_ms": (C.c_double, [C.c_void_p]),
    "nb_hip_ensemble_trace_mode": (None, [C.c_void_p, C.c_int]),
    "nb_hip_ensemble_last_trace_info": (None, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "nb_hip_ensemble_render_mode": (None, [C.c_void_p, C.c_int]),
    "nb_hip_ensemble_last_render_info": (None, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "nb_hip_ensemble_last_render_ms": (C.c_double, [C.c_void_p]),
    "nb_hip_last_leapfrog_info": (None, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "nb_hip_ensemble_last_leapfrog_info": (None, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "nb_hip_live_resources": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
}
PUBLIC_KNOBS = ("variant", "graph", "timing", "overlap", "sharded_graph")   # nb_hip_configure; everything else is a tuning hook

# include/nbody.h + include/galaxy.h + include/nbody_diag.h + include/nbody_batch.h + include/nbody_batch_diag.h +
# include/nbody_render.h + include/nbody_batch_render.h + include/nbody_batch_ragged.h + include/nbody_field.h + include/nbody_gravity.h +
# include/nbody_adaptive.h + include/nbody_leapfrog.h + include/nbody_batch_field.h + include/nbody_tidal.h + include/nbody_batch_tidal.h +
# include/nbody_profile.h + include/nbody_batch_profile.h + include/nbody_paircount.h + include/nbody_batch_paircount.h +
# include/nbody_neighbour.h + include/nbody_batch_neighbour.h
NBODY_API = {
    "CreateWorld": (C.c_void_p, [C.c_void_p, C.c_uint32]),
    "DestroyWorld": (None, [C.c_void_p]),
    "GetWorldParticles": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "UpdateWorld_CPU": (None, [C.c_void_p, C.c_float, C.c_uint32]),
    "UpdateWorld_GPU": (None, [C.c_void_p, C.c_float, C.c_uint32]),
    "CreateWorldSharded": (C.c_void_p, [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "CreateWorldShardedWith": (C.c_void_p, [C.c_void_p, C.c_uint32, C.c_int, C.c_int, ALLGATHER_FN, C.c_void_p]),
    "CreateWorldShardedDirect": (C.c_void_p, [C.c_void_p, C.c_uint32, C.c_int, C.c_int, ALLGATHER_FN, C.c_void_p]),
    "GetWorldPipeline": (C.c_void_p, [C.c_void_p]),
    "MakeGalaxies": (C.c_void_p, [C.c_uint32, C.c_uint32]),
    "MakeGalaxiesSeeded": (C.c_void_p, [C.c_uint32, C.c_uint32, C.c_uint64]),
    "GetWorldEnergy": (None, [C.c_void_p, C.POINTER(WorldEnergy)]),
    "GetWorldPotential": (None, [C.c_void_p, C.c_void_p]),
    # include/nbody_render.h
    "DefaultRenderPalette": (None, [C.POINTER(RenderPalette)]),
    "GetWorldBounds": (None, [C.c_void_p, C.c_void_p]),
    "FitWorldView": (None, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RenderView)]),
    "RenderWorldCounts": (None, [C.c_void_p, C.POINTER(RenderView), C.c_void_p]),
    "RenderWorld": (None, [C.c_void_p, C.POINTER(RenderView), C.POINTER(RenderPalette), C.c_void_p]),
    # include/nbody_field.h
    "GetWorldPotentialAt": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "RenderWorldPotential": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    # include/nbody_gravity.h
    "GetWorldAccelerationAt": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "RenderWorldAcceleration": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    # include/nbody_tidal.h
    "GetWorldTidalAt": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "RenderWorldTidal": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    # include/nbody_profile.h, include/nbody_batch_profile.h
    "GetWorldProfile": (None, [C.c_void_p, C.POINTER(WorldProfileSpec), C.c_void_p, C.c_void_p]),
    "GetWorldBatchProfile": (None, [C.c_void_p, C.POINTER(WorldProfileSpec), C.c_uint32, C.c_void_p, C.c_void_p]),
    # include/nbody_paircount.h, include/nbody_batch_paircount.h
    "GetWorldPairCounts": (None, [C.c_void_p, C.POINTER(WorldPairSpec), C.c_void_p, C.c_void_p]),
    "GetWorldBatchPairCounts": (None, [C.c_void_p, C.POINTER(WorldPairSpec), C.c_void_p, C.c_void_p]),
    # include/nbody_neighbour.h, include/nbody_batch_neighbour.h
    "GetWorldNeighbours": (None, [C.c_void_p, C.POINTER(WorldNeighbourSpec), C.c_void_p, C.c_void_p, C.c_void_p]),
    "GetWorldBatchNeighbours": (None, [C.c_void_p, C.POINTER(WorldNeighbourSpec), C.c_void_p, C.c_void_p, C.c_void_p]),
    # include/nbody_batch.h
    "CreateWorldBatch": (C.c_void_p, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "DestroyWorldBatch": (None, [C.c_void_p]),
    "GetWorldBatchParticles": (C.c_void_p, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "UpdateWorldBatch_GPU": (None, [C.c_void_p, C.c_float, C.c_uint32]),
    "UpdateWorldBatch_GPU_dts": (None, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32]),
    # include/nbody_batch_diag.h
    "GetWorldBatchEnergy": (None, [C.c_void_p, C.POINTER(WorldEnergy)]),
    "GetWorldBatchPotential": (None, [C.c_void_p, C.c_void_p]),
    # include/nbody_batch_trace.h
    "UpdateWorldBatch_GPU_Traced": (None, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p]),
    "UpdateWorldBatch_GPU_Traced_dts": (None, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_void_p]),
    # include/nbody_batch_render.h
    "GetWorldBatchBounds": (None, [C.c_void_p, C.c_void_p]),
    "FitWorldBatchViews": (None, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RenderView)]),
    "RenderWorldBatchCounts": (None, [C.c_void_p, C.POINTER(RenderView), C.c_void_p]),
    "RenderWorldBatch": (None, [C.c_void_p, C.POINTER(RenderView), C.POINTER(RenderPalette), C.c_void_p]),
    # include/nbody_batch_ragged.h
    "CreateWorldBatchRagged": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]),
    # include/nbody_batch_field.h
    "GetWorldBatchPotentialAt": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "RenderWorldBatchPotential": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    "GetWorldBatchAccelerationAt": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "RenderWorldBatchAcceleration": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    # include/nbody_batch_tidal.h
    "GetWorldBatchTidalAt": (None, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "RenderWorldBatchTidal": (None, [C.c_void_p, C.POINTER(RenderView), C.c_float, C.c_void_p]),
    # include/nbody_adaptive.h
    "UpdateWorld_GPU_Adaptive": (None, [C.c_void_p, C.c_uint32, C.POINTER(NbAdaptive), C.c_void_p, C.POINTER(NbAdaptiveResult)]),
    "UpdateWorld_CPU_Adaptive": (None, [C.c_void_p, C.c_uint32, C.POINTER(NbAdaptive), C.c_void_p, C.POINTER(NbAdaptiveResult)]),
    "GetWorldTimestep": (None, [C.c_void_p, C.POINTER(NbAdaptive), C.POINTER(C.c_float)]),
    "AdvanceWorld_GPU": (None, [C.c_void_p, C.c_double, C.POINTER(NbAdaptive), C.c_uint32, C.c_void_p, C.POINTER(NbAdaptiveResult)]),
    "UpdateWorldBatch_GPU_Adaptive": (None, [C.c_void_p, C.c_uint32, C.POINTER(NbAdaptive), C.c_void_p, C.c_void_p]),
    "AdvanceWorldBatch_GPU": (None, [C.c_void_p, C.c_double, C.POINTER(NbAdaptive), C.c_uint32, C.c_void_p, C.c_void_p]),
    # include/nbody_leapfrog.h
    "UpdateWorld_GPU_Leapfrog": (None, [C.c_void_p, C.c_float, C.c_uint32]),
    "UpdateWorld_CPU_Leapfrog": (None, [C.c_void_p, C.c_float, C.c_uint32]),
    "UpdateWorldBatch_GPU_Leapfrog": (None, [C.c_void_p, C.c_float, C.c_uint32]),
    "UpdateWorldBatch_GPU_Leapfrog_dts": (None, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32]),
}

_hip = None
_nbody = None


def _bind(lib, api):
    for name, (res, args) in api.items():
        f = getattr(lib, name)  # AttributeError if the library does not export it
        f.restype = res
        f.argtypes = args
    return lib


def _build_if_missing(path):
    """A missing library is built once, loudly; there is no other implementation to fall back to."""
    if os.path.exists(path) or os.environ.get("NBODY_HIP_SO"):
        return
    import sys
    from . import build as _build
    print(f"[nbody_amd] {path} missing: building the product libraries (hipcc, gfx950)", file=sys.stderr, flush=True)
    _build.build_product()


def hip_lib():
    """libnbody_hip.so, loaded once.  Raises OSError when it cannot be built or loaded."""
    global _hip
    if _hip is None:
        _build_if_missing(HIP_SO)
        if not os.path.exists(HIP_SO):
            raise OSError(f"{HIP_SO} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _hip = _bind(_bind(C.CDLL(HIP_SO, mode=C.RTLD_GLOBAL), HIP_API), TUNE_API)
    return _hip


def nbody_lib():
    """libnbody.so (World API), loaded once; pulls libnbody_hip.so in first."""
    global _nbody
    if _nbody is None:
        hip_lib()
        _build_if_missing(NBODY_SO)
        if not os.path.exists(NBODY_SO):
            raise OSError(f"{NBODY_SO} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _nbody = _bind(C.CDLL(NBODY_SO, mode=C.RTLD_GLOBAL), NBODY_API)
    return _nbody


def as_particles(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError("particles must have shape (n, 8)")
    return a


def as_points(points):
    """(n, 2) float32, contiguous: the probe points of include/nbody_field.h."""
    a = np.ascontiguousarray(points, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("points must have shape (n, 2)")
    return a


def device_count():
    return int(hip_lib().nb_hip_device_count())


def live_resources():
    """nb_hip_live_resources (tuning hook): (device allocations, events) the library holds right now; needs no GPU."""
    buffers, events = C.c_uint32(0), C.c_uint32(0)
    hip_lib().nb_hip_live_resources(C.byref(buffers), C.byref(events))
    return int(buffers.value), int(events.value)


def device_info():
    buf = C.create_string_buffer(256)
    hip_lib().nb_hip_device_info(buf, 256)
    return buf.value.decode()


def probe_clock(target_ms=40.0):
    """include/nbody_hip.h nb_hip_probe_clock: the shader clock held under the step kernels' instruction mix."""
    v = [C.c_double(0.0) for _ in range(5)]
    waves = hip_lib().nb_hip_probe_clock(float(target_ms), *[C.byref(x) for x in v])
    return {"clock_ghz": v[0].value, "clock_ghz_min": v[1].value, "clock_ghz_max": v[2].value,
            "cycles_per_wave_interaction": v[3].value, "elapsed_ms": v[4].value, "waves": int(waves)}


def clock_sampler_begin(period_ms=0.5, max_ms=6000.0):
    """include/nbody_hip.h nb_hip_clock_sampler_begin: sample the shader clock while other kernels run."""
    return int(hip_lib().nb_hip_clock_sampler_begin(float(period_ms), float(max_ms)))


def clock_sampler_end():
    ghz, lo, hi, span = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    per_xcd, profile = (C.c_double * 8)(), (C.c_double * 10)()
    dropped = C.c_uint32(0)
    n = hip_lib().nb_hip_clock_sampler_end(C.byref(ghz), C.byref(lo), C.byref(hi), per_xcd, profile, C.byref(span), C.byref(dropped))
    return {"clock_ghz": ghz.value, "clock_ghz_min": lo.value, "clock_ghz_max": hi.value, "per_xcd_ghz": [float(v) for v in per_xcd],
            "profile_ghz": [float(v) for v in profile], "span_ms": span.value, "intervals": int(n), "dropped_intervals": int(dropped.value)}


def preflight_peers(max_devices=16):
    """include/nbody_hip.h nb_hip_preflight_peers: (visible devices, hipDeviceCanAccessPeer row of this process' device)."""
    row = (C.c_int * max_devices)()
    count = int(hip_lib().nb_hip_preflight_peers(row, max_devices))
    return count, [int(v) for v in row[:min(count, max_devices)]]


def preflight_ipc_export(tag):
    """(hipError_t, 64-byte IPC handle of a device word holding `tag`)."""
    buf = (C.c_ubyte * 64)()
    rc = int(hip_lib().nb_hip_preflight_ipc_export(buf, int(tag) & 0xffffffff))
    return rc, bytes(buf)


def preflight_ipc_open(handle, expect_tag):
    """(0 / hipError_t / -1, host ms) of mapping a peer's exported word, reading it and unmapping."""
    ms = C.c_double(0.0)
    buf = (C.c_ubyte * 64).from_buffer_copy(handle)
    rc = int(hip_lib().nb_hip_preflight_ipc_open(buf, int(expect_tag) & 0xffffffff, C.byref(ms)))
    return rc, float(ms.value)


def hip_error_string(code):
    return hip_lib().nb_hip_error_string(int(code)).decode(errors="replace")


def shard_plan(total_len, mass_len, rank, nranks):
    p = hip_lib().nb_hip_shard_plan(total_len, mass_len, rank, nranks)
    return {n: int(getattr(p, n)) for n, _ in NbShardPlan._fields_}


def plan_launch(n_recv, n_src, compute_units=256):
    """The classic (k, w, split, unit) plan, plus "lanes" / "lanes_w": whether an all-auto unsharded step of that size
    runs as a lane-split launch instead (lanes > 1) and with how many waves per workgroup."""
    k, w, sp, g, lw = C.c_int(), C.c_int(), C.c_int(), C.c_uint32(), C.c_int()
    hip_lib().nb_hip_plan_launch(n_recv, n_src, compute_units, C.byref(k), C.byref(w), C.byref(sp), C.byref(g))
    lanes = int(hip_lib().nb_hip_plan_launch_lanes(n_recv, n_src, C.byref(lw)))
    return {"k": k.value, "w": w.value, "split": sp.value, "workgroups": g.value,
            "unit": int(hip_lib().nb_hip_plan_launch_unit(n_recv, n_src, compute_units)), "lanes": lanes, "lanes_w": lw.value,
            "fused_finish": int(hip_lib().nb_hip_plan_fused_finish(n_recv, n_src, compute_units))}


def plan_deal(n_recv, n_src, compute_units=256):
    """tuning hook: whether "deal" = 2 deals the step launches of an unsharded world of that size (host arithmetic)."""
    return bool(hip_lib().nb_hip_plan_deal(n_recv, n_src, compute_units))


def deal_item(ticket, tiles, split):
    """tuning hook: the (receiver tile, source part) a dealt launch's ticket stands for, or None past the last item."""
    tile, part = C.c_uint32(0), C.c_uint32(0)
    live = hip_lib().nb_hip_deal_item(ticket, tiles, split, C.byref(tile), C.byref(part))
    return (int(tile.value), int(part.value)) if live else None


def comm_unique_id():
    buf = (C.c_ubyte * UNIQUE_ID_BYTES)()
    hip_lib().nb_hip_comm_unique_id(buf)
    return bytes(buf)


class SimPipeline:
    """The inner seam (reference src/lib/sim_gpu.h:21-36) as an object.

    `particles` passed to set_data must already be partitioned (mass > 0 first) with
    `mass_len` massive ones, exactly what reference src/lib/world.c:32-58 hands its backend.
    """

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

    def energy(self):
        """nb_hip_energy: kinetic / potential / total energy, mass, momentum, angular momentum, centre of mass (float64)."""
        e = WorldEnergy()
        hip_lib().nb_hip_energy(self._h, C.byref(e))
        return e.as_dict()

    def potential(self):
        """nb_hip_potential: Phi_i of every particle (float32, partitioned order)."""
        out = np.empty(self.total_len, dtype=np.float32)
        hip_lib().nb_hip_potential(self._h, out.ctypes.data)
        return out

    def potential_at(self, points, softening):
        """nb_hip_potential_at: Phi at the (n, 2) points with one softening (include/nbody_field.h), float32 (n,)."""
        pts = as_points(points)
        out = np.empty(pts.shape[0], dtype=np.float32)
        hip_lib().nb_hip_potential_at(self._h, pts.ctypes.data, pts.shape[0], softening, out.ctypes.data)
        return out

    def potential_map(self, view, softening):
        """nb_hip_potential_map: Phi at every pixel centre of the view, float32 (height, width)."""
        out = np.empty((view.height, view.width), dtype=np.float32)
        hip_lib().nb_hip_potential_map(self._h, C.byref(view), softening, out.ctypes.data)
        return out

    def acceleration_at(self, points, softening):
        """nb_hip_acceleration_at: g at the (n, 2) points with one softening (include/nbody_gravity.h), float32 (n, 2)."""
        pts = as_points(points)
        out = np.empty((pts.shape[0], 2), dtype=np.float32)
        hip_lib().nb_hip_acceleration_at(self._h, pts.ctypes.data, pts.shape[0], softening, out.ctypes.data)
        return out

    def acceleration_map(self, view, softening):
        """nb_hip_acceleration_map: g at every pixel centre of the view, float32 (height, width, 2)."""
        out = np.empty((view.height, view.width, 2), dtype=np.float32)
        hip_lib().nb_hip_acceleration_map(self._h, C.byref(view), softening, out.ctypes.data)
        return out

    def pair_counts(self, edges, classes=("mm",), return_unplaced=False):
        """nb_hip_pair_counts: the pairs of particles per row of separations and per class (include/nbody_paircount.h), uint64
        (bins + 2, 3) with the columns (massive-massive, massive-massless, massless-massless); row 0 lies inside edges[0], row
        bins + 1 at or beyond edges[-1].  classes: any subset of "mm", "mt", "tt", or "all"; a class not asked for is zeros and is
        never evaluated.  With return_unplaced also the pairs per class whose squared separation is NaN.  Every count is exact:
        device, host and numpy agree bit for bit.  nb.profile_edges makes edges, nb.pair_curves reads the result."""
        return _pair_counts(hip_lib().nb_hip_pair_counts, self._h, None, edges, classes, return_unplaced)

    def neighbours(self, radius=None, receivers="all", sources="all"):
        """nb_hip_neighbours: the nearest neighbour of every particle (include/nbody_neighbour.h): (q, index), or (q, index, count)
        when a radius is given -- q float32, the squared distance to the closest other particle of `sources` (+inf without one);
        index uint32, which one (the smallest index among equal q; nb.NB_NEIGH_NONE without one); count uint32, how many lie
        within `radius`.  receivers / sources: "massive", "massless" or "all"; a particle that is no receiver gets
        (+inf, NONE, 0) and a class that is neither is never read.  Device, host and numpy agree bit for bit.
        nb.neighbour_distance and nb.closest_pairs read the result.  Shapes (N,)."""
        return _neighbours(hip_lib().nb_hip_neighbours, self.total_len, None, radius, receivers, sources)(self._h)

    def profile(self, edges, centre=(0.0, 0.0), centre_velocity=(0.0, 0.0), weights="mass", return_unplaced=False):
        """nb_hip_profile: the annulus moments about `centre` moving with `centre_velocity` (include/nbody_profile.h), float64
        (bins + 2, 6) with the columns (count, S, I, L, W, K); row 0 lies inside edges[0], row bins + 1 at or beyond edges[-1].
        weights: "mass" (massive particles, weight m) or "number" (all particles, weight 1).  With return_unplaced also the number
        of particles whose squared radius is NaN.  A natural centre: energy()["center_of_mass"] and momentum / mass (vel is used
        as stored, the caveat of include/nbody_diag.h).  nb.profile_curves / nb.lagrangian_radii read the result."""
        e, bins, c, mode = _profile_args(edges, centre, centre_velocity, weights)
        out, lost = np.empty((bins + 2, NB_PROFILE_QTY), dtype=np.float64), np.zeros(1, dtype=np.uint32)
        hip_lib().nb_hip_profile(self._h, e.ctypes.data, bins, c.ctypes.data, mode, out.ctypes.data, lost.ctypes.data)
        return (out, int(lost[0])) if return_unplaced else out

    def tidal_at(self, points, softening):
        """nb_hip_tidal_at: the tidal tensor dg/dp at the (n, 2) points with one softening (include/nbody_tidal.h), float32
        (n, 3) in the order (xx, xy, yy)."""
        pts = as_points(points)
        out = np.empty((pts.shape[0], 3), dtype=np.float32)
        hip_lib().nb_hip_tidal_at(self._h, pts.ctypes.data, pts.shape[0], softening, out.ctypes.data)
        return out

    def tidal_map(self, view, softening):
        """nb_hip_tidal_map: the tidal tensor at every pixel centre of the view, float32 (height, width, 3)."""
        out = np.empty((view.height, view.width, 3), dtype=np.float32)
        hip_lib().nb_hip_tidal_map(self._h, C.byref(view), softening, out.ctypes.data)
        return out

    def last_diag_ms(self):
        """tuning hook: device ms of the kernels of the last energy() / potential() / potential_at() / potential_map() /
        acceleration_at() / acceleration_map() / tidal_at() / tidal_map() / profile() / pair_counts() / neighbours(); 0.0 after a
        call that had nothing to launch."""
        return float(hip_lib().nb_hip_last_diag_ms(self._h))

    def bounds(self):
        """nb_hip_bounds: float32 [min.x, min.y, max.x, max.y] over the particles with finite x and y."""
        out = np.empty(4, dtype=np.float32)
        hip_lib().nb_hip_bounds(self._h, out.ctypes.data)
        return out

    def render_counts(self, view):
        """nb_hip_render_counts: uint32 (3, height, width), particles of each class covering each pixel."""
        out = np.empty((3, view.height, view.width), dtype=np.uint32)
        hip_lib().nb_hip_render_counts(self._h, C.byref(view), out.ctypes.data)
        return out

    def render(self, view, palette=None):
        """nb_hip_render_rgba: uint8 (height, width, 4); palette None = DefaultRenderPalette."""
        out = np.empty((view.height, view.width, 4), dtype=np.uint8)
        pal = palette if palette is not None else default_palette()
        hip_lib().nb_hip_render_rgba(self._h, C.byref(view), C.byref(pal), out.ctypes.data)
        return out

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


def as_ensemble(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 8:
        raise ValueError("an ensemble must have shape (members, n, 8)")
    return a


def _packed(members):
    """a list of (N_b, 8) arrays -> (one packed float32 (sum N_b, 8) array, uint32 sizes)"""
    parts = [as_particles(m) for m in members]
    sizes = np.array([p.shape[0] for p in parts], dtype=np.uint32)
    flat = np.concatenate(parts, axis=0) if parts else np.zeros((0, 8), np.float32)
    return np.ascontiguousarray(flat, dtype=np.float32), sizes


def _unpacked(flat, offsets):
    return [flat[int(offsets[b]):int(offsets[b + 1])].copy() for b in range(len(offsets) - 1)]


def _dt_array(dts, count):
    a = np.ascontiguousarray(dts, dtype=np.float32)
    if a.shape != (count,):
        raise ValueError(f"expected {count} step sizes")
    return a


def _member_points(points, count):
    """(n, 2) points for every member, or (count, n, 2) with one set per member -> contiguous float32 (count, n, 2)."""
    a = np.asarray(points, dtype=np.float32)
    if a.ndim == 2:
        a = np.broadcast_to(a, (count,) + a.shape)
    if a.ndim != 3 or a.shape[0] != count or a.shape[2] != 2:
        raise ValueError(f"points must have shape (n, 2) or ({count}, n, 2)")
    return np.ascontiguousarray(a)


def _ensemble_field(fn, handle, count, components, softening, points=None, views=None):
    """One of the six field calls of an ensemble (fn: nb_hip_ensemble_* of a SimBatch, include/nbody_batch_field.h of a
    WorldBatch) at `points` or, where they are None, under `views`: float32 (B, n) / (B, h, w), with a last axis of 2 for g
    and of 3 for the tidal tensor."""
    tail = (components,) if components > 1 else ()
    if points is not None:
        pts = _member_points(points, count)
        out = np.empty((count, pts.shape[1]) + tail, dtype=np.float32)
        fn(handle, pts.ctypes.data, pts.shape[1], softening, out.ctypes.data)
        return out
    arr, w, h = _view_array(views, count)
    out = np.empty((count, h, w) + tail, dtype=np.float32)
    fn(handle, arr, softening, out.ctypes.data)
    return out


def _view_array(views, count):
    """One RenderView for every member, or a sequence of `count` of them -> (RenderView[count], width, height)."""
    if isinstance(views, RenderView):
        views = [views] * count
    views = list(views)
    if len(views) != count:
        raise ValueError(f"expected one RenderView or {count} of them")
    arr = (RenderView * count)()
    for b, v in enumerate(views):
        C.memmove(C.byref(arr[b]), C.byref(v), C.sizeof(RenderView))
    return arr, int(arr[0].width), int(arr[0].height)


def _profile_args(edges, centre, centre_velocity, weights, count=None):
    """(edges float32 (bins + 1,), bins, centres float32 (4,) or (count, 4) as (cx, cy, ux, uy), weights as the C enum)."""
    e = np.ascontiguousarray(edges, dtype=np.float32)
    if e.ndim != 1 or e.shape[0] < 2:
        raise ValueError("edges must be a sequence of at least two radii")
    modes = {"mass": NB_PROFILE_BY_MASS, "number": NB_PROFILE_BY_NUMBER, NB_PROFILE_BY_MASS: NB_PROFILE_BY_MASS,
             NB_PROFILE_BY_NUMBER: NB_PROFILE_BY_NUMBER}
    if isinstance(weights, (str, int)) and weights in modes:
        mode = modes[weights]
    elif isinstance(weights, (int, np.integer)):
        mode = int(weights)          # the library names the fault
    else:
        raise ValueError('weights must be "mass" or "number"')
    c, u = np.asarray(centre, dtype=np.float32), np.asarray(centre_velocity, dtype=np.float32)
    if count is None:
        if c.shape != (2,) or u.shape != (2,):
            raise ValueError("centre and centre_velocity must have shape (2,)")
        return e, e.shape[0] - 1, np.ascontiguousarray(np.concatenate([c, u])), mode
    for a in (c, u):
        if a.shape != (2,) and a.shape != (count, 2):
            raise ValueError(f"centre and centre_velocity must have shape (2,) or ({count}, 2)")
    both = np.empty((count, 4), dtype=np.float32)
    both[:, 0:2], both[:, 2:4] = c, u
    return e, e.shape[0] - 1, both, mode


def _profile_specs(e, bins, centres, mode):
    """One WorldProfileSpec per row of centres (count, 4), all pointing at the edges e."""
    specs = (WorldProfileSpec * centres.shape[0])()
    for b, row in enumerate(centres):
        specs[b].edges, specs[b].bins, specs[b].weights = e.ctypes.data, bins, mode
        specs[b].centre[0], specs[b].centre[1] = row[0], row[1]
        specs[b].centre_velocity[0], specs[b].centre_velocity[1] = row[2], row[3]
    return specs


def _pair_args(edges, classes):
    """(edges float32 (bins + 1,), bins, classes as the C bit mask)."""
    e = np.ascontiguousarray(edges, dtype=np.float32)
    if e.ndim != 1 or e.shape[0] < 2:
        raise ValueError("edges must be a sequence of at least two radii")
    names = {"mm": NB_PAIRS_MM, "mt": NB_PAIRS_MT, "tt": NB_PAIRS_TT, "all": NB_PAIRS_ALL}
    if isinstance(classes, (int, np.integer)) and not isinstance(classes, bool):
        return e, e.shape[0] - 1, int(classes) & 0xffffffff          # the library names the fault
    if isinstance(classes, str):
        classes = (classes,)
    mask = 0
    try:
        for c in classes:
            mask |= names[c]
    except (KeyError, TypeError):
        raise ValueError('classes must be a subset of "mm", "mt", "tt", or "all"') from None
    if mask == 0:
        raise ValueError('classes must name at least one of "mm", "mt", "tt"')
    return e, e.shape[0] - 1, mask


def _pair_counts(call, handle, count, edges, classes, return_unplaced, spec=False):
    """One pair-count call of the seam (edges, bins, classes) or of the World layer (a WorldPairSpec): uint64 (bins + 2, 3), or
    (count, bins + 2, 3) for an ensemble."""
    e, bins, mask = _pair_args(edges, classes)
    shape = (bins + 2, NB_PAIRS_COLUMNS) if count is None else (count, bins + 2, NB_PAIRS_COLUMNS)
    out, lost = np.zeros(shape, dtype=np.uint64), np.zeros(shape[:-2] + (NB_PAIRS_COLUMNS,), dtype=np.uint64)
    if spec:
        call(handle, C.byref(WorldPairSpec(e.ctypes.data, bins, mask)), out.ctypes.data, lost.ctypes.data)
    else:
        call(handle, e.ctypes.data, bins, mask, out.ctypes.data, lost.ctypes.data)
    return (out, lost) if return_unplaced else out


def _neigh_mask(name, what):
    names = {"massive": NB_NEIGH_MASSIVE, "massless": NB_NEIGH_MASSLESS, "all": NB_NEIGH_ALL}
    if isinstance(name, (int, np.integer)) and not isinstance(name, bool):
        return int(name) & 0xffffffff          # the library names the fault
    try:
        return names[name]
    except (KeyError, TypeError):
        raise ValueError(f'{what} must be "massive", "massless" or "all"') from None


def _neighbours(call, entries, offsets, radius, receivers, sources, spec=False, shape=None):
    """One neighbour call of the seam (receivers, sources, radius) or of the World layer (a WorldNeighbourSpec) over `entries`
    particles: a function of the handle that returns (q, index[, count]) -- flat, reshaped to `shape`, or split at `offsets`."""
    r, s = _neigh_mask(receivers, "receivers"), _neigh_mask(sources, "sources")
    h = 0.0 if radius is None else float(radius)

    def run(handle):
        q, index = np.empty(entries, dtype=np.float32), np.empty(entries, dtype=np.uint32)
        count = None if radius is None else np.empty(entries, dtype=np.uint32)
        where = None if count is None else count.ctypes.data
        if spec:
            call(handle, C.byref(WorldNeighbourSpec(r, s, h)), q.ctypes.data, index.ctypes.data, where)
        else:
            call(handle, r, s, h, q.ctypes.data, index.ctypes.data, where)
        out = (q, index) if count is None else (q, index, count)
        if offsets is not None:
            return tuple(_unpacked(a, offsets) for a in out)
        return tuple(a.reshape(shape) for a in out) if shape is not None else out
    return run


def neighbour_distance(q):
    """float64 sqrt(q) of the q of .neighbours(): the distance to the nearest neighbour, +inf kept where there is none."""
    return np.sqrt(np.asarray(q, dtype=np.float64))


def closest_pairs(q, index, k=1):
    """The k closest unordered pairs among the nearest-neighbour links of one world's .neighbours(): a list of (i, j, q) with
    i < j, sorted by (q, i, j); a mutual pair appears once, a particle without a neighbour in none.  The first row is the closest
    encounter of the world: the two particles that set an adaptive step."""
    q, index = np.asarray(q, dtype=np.float32), np.asarray(index, dtype=np.uint32)
    if q.ndim != 1 or index.shape != q.shape:
        raise ValueError("q and index must be the (N,) arrays of one world")
    if k < 0:
        raise ValueError("k must not be negative")
    has = np.nonzero(index != NB_NEIGH_NONE)[0]
    pairs = {(min(int(i), int(index[i])), max(int(i), int(index[i]))): float(q[i]) for i in has}
    rows = sorted((v, i, j) for (i, j), v in pairs.items())[:k]
    return [(i, j, v) for v, i, j in rows]


def pair_curves(rows, edges):
    """What the counts of .pair_counts() say, per class (rows (..., bins + 2, 3)).  A dict of float64 arrays: r_mid and area
    (bins,) of the caller's annuli; density (..., bins, 3) = pairs of the bin per unit annulus area per pair of the class -- the
    radial pair density a correlation function is formed from (divide by that of an unclustered set); cumulative
    (..., bins + 1, 3) = the fraction of the class's pairs within each edge.  NaN where a class has no pair.  The class totals are
    the sums over all rows: unplaced pairs (a NaN separation) are not among them."""
    r = np.asarray(rows, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    if r.ndim < 2 or r.shape[-1] != NB_PAIRS_COLUMNS or r.shape[-2] != e.shape[0] + 1:
        raise ValueError("rows must have shape (..., len(edges) + 1, 3)")
    area = np.pi * (e[1:] ** 2 - e[:-1] ** 2)
    total = r.sum(axis=-2, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        density = np.where(total > 0, r[..., 1:-1, :] / area[:, None] / total, np.nan)
        cumulative = np.where(total > 0, np.cumsum(r[..., :-1, :], axis=-2) / total, np.nan)
    return {"r_mid": 0.5 * (e[1:] + e[:-1]), "area": area, "density": density, "cumulative": cumulative}


def profile_edges(r_min, r_max, bins, log=False):
    """bins + 1 float32 radii from r_min to r_max, equally spaced in r or, with log, in log r (r_min > 0 then)."""
    if bins < 1 or bins > NB_PROFILE_MAX_BINS:
        raise ValueError(f"bins must be 1 .. {NB_PROFILE_MAX_BINS}")
    if not (0.0 <= r_min < r_max) or (log and not r_min > 0.0):
        raise ValueError("need 0 <= r_min < r_max, and r_min > 0 for logarithmic bins")
    e = (np.geomspace(r_min, r_max, bins + 1) if log else np.linspace(r_min, r_max, bins + 1)).astype(np.float32)
    if not np.all(np.diff(e) > 0):
        raise ValueError("the edges are not strictly increasing in float32: fewer bins or a wider range")
    return e


def profile_curves(rows, edges):
    """What the annulus moments of .profile() say, per bin of `edges` (rows 1 .. bins of rows (..., bins + 2, 6); the rows
    inside edges[0] and beyond edges[-1] only enter `enclosed`).  A dict of float64 arrays (..., bins), NaN where a bin's S is
    0: r_mid, area, surface_density = S / area, enclosed (the cumulative S up to the bin's outer edge, row 0 included),
    r_rms = sqrt(I / S), omega = L / I, v_rot = omega r_rms, expansion = W / I, v_rad = expansion r_rms and
    sigma2 = max(0, K - L^2 / I - W^2 / I) / S (the velocity dispersion, both components together)."""
    r = np.asarray(rows, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    if r.shape[-1:] != (NB_PROFILE_QTY,) or r.ndim < 2 or r.shape[-2] != e.shape[0] + 1:
        raise ValueError("rows must have shape (..., len(edges) + 1, 6)")
    S, I, L, W, K = (r[..., 1:-1, c] for c in range(1, 6))
    area = np.pi * (e[1:] ** 2 - e[:-1] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        empty = S == 0
        nan = lambda a: np.where(empty, np.nan, a)
        r_rms = np.sqrt(I / S)
        omega, expansion = L / I, W / I
        out = {
            "r_mid": 0.5 * (e[1:] + e[:-1]) + np.zeros_like(S),
            "area": area + np.zeros_like(S),
            "surface_density": nan(S / area),
            "enclosed": np.cumsum(r[..., :-1, 1], axis=-1)[..., 1:],
            "r_rms": nan(r_rms),
            "omega": nan(omega),
            "v_rot": nan(omega * r_rms),
            "expansion": nan(expansion),
            "v_rad": nan(expansion * r_rms),
            "sigma2": nan(np.maximum(0.0, K - L * L / I - W * W / I) / S),
        }
    return out


def lagrangian_radii(rows, edges, fractions):
    """The radii that enclose the given fractions of the total S (all rows) of one profile (bins + 2, 6): the enclosed mass
    inverted, the mass of a bin taken as uniform in area, that is linear in r^2.  NaN for a fraction reached inside edges[0]
    or only beyond edges[-1]."""
    r = np.asarray(rows, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    if r.shape != (e.shape[0] + 1, NB_PROFILE_QTY):
        raise ValueError("rows must have shape (len(edges) + 1, 6)")
    f = np.atleast_1d(np.asarray(fractions, dtype=np.float64))
    at_edge = np.cumsum(r[:-1, 1])          # the S inside edges[t]
    target = f * r[:, 1].sum()
    out = np.full(f.shape, np.nan)
    for i, m in enumerate(target):
        if not (at_edge[0] <= m <= at_edge[-1]) or not np.isfinite(m):
            continue
        t = int(np.searchsorted(at_edge, m, side="left"))       # the first edge with at_edge[t] >= m
        if t == 0 or at_edge[t] == at_edge[t - 1]:
            out[i] = e[t]
            continue
        x = (m - at_edge[t - 1]) / (at_edge[t] - at_edge[t - 1])
        out[i] = np.sqrt(e[t - 1] ** 2 + x * (e[t] ** 2 - e[t - 1] ** 2))
    return out if np.ndim(fractions) else out[0]


def tidal_invariants(t):
    """(trace, lambda_plus, lambda_minus) of tidal tensors t (..., 3) in the order (xx, xy, yy), float64: the in-plane trace
    xx + yy and the eigenvalues trace / 2 +- sqrt(((xx - yy) / 2)^2 + xy^2), lambda_plus >= lambda_minus.  A positive
    eigenvalue stretches a small body along its axis, a negative one compresses it."""
    a = np.asarray(t, dtype=np.float64)
    if a.shape[-1:] != (3,):
        raise ValueError("tidal tensors must have a last axis of 3: (xx, xy, yy)")
    xx, xy, yy = a[..., 0], a[..., 1], a[..., 2]
    trace = xx + yy
    root = np.sqrt(((xx - yy) / 2.0) ** 2 + xy ** 2)
    return trace, trace / 2.0 + root, trace / 2.0 - root


def contact_sheet(frames, columns):
    """(B, h, w, 4) frames -> one (rows * h, columns * w, 4) image, member b in row b // columns, column b % columns;
    cells without a member are zero."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or columns < 1:
        raise ValueError("frames must have shape (B, h, w, channels) and columns must be at least 1")
    count, h, w, ch = frames.shape
    rows = -(-count // columns)
    sheet = np.zeros((rows * columns, h, w, ch), dtype=frames.dtype)
    sheet[:count] = frames
    return sheet.reshape(rows, columns, h, w, ch).transpose(0, 2, 1, 3, 4).reshape(rows * h, columns * w, ch)


class SimBatch:
    """include/nbody_hip.h SimBatch: B independent worlds of the same size, stepped together (nb_hip_batch_*).

    Particles are float32 arrays of shape (B, n, 8), every member already partitioned (mass > 0 first) with
    `mass_len[b]` massive ones.  Member b ends bit-identical to the same particles alone in a SimPipeline pinned to
    launch_shape().

    SimBatch.ragged(total_lens, mass_lens) makes an ensemble whose members differ in size (nb_hip_ragged_create): set_data
    takes and get_data() / potential() return a LIST of per-member arrays, everything else keeps its shape; member b is
    bit-identical to the same particles as the single member of SimBatch(total_lens[b], [mass_lens[b]])."""

    is_ragged = False

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

    def energy(self):
        """nb_hip_ensemble_energy: one dict per member (WorldEnergy.as_dict), each bit-identical to SimPipeline.energy() of
        the same particles; two launches for the whole ensemble, no read-back of the particles."""
        out = (WorldEnergy * self.count)()
        hip_lib().nb_hip_ensemble_energy(self._h, out)
        return [e.as_dict() for e in out]

    def potential(self):
        """nb_hip_ensemble_potential: Phi_i of every particle of every member, float32 (B, n), partitioned order; ragged: a
        list of B float32 (N_b,) arrays."""
        if self.is_ragged:
            flat = np.empty(int(self.offsets[-1]), dtype=np.float32)
            hip_lib().nb_hip_ensemble_potential(self._h, flat.ctypes.data)
            return _unpacked(flat, self.offsets)
        out = np.empty((self.count, self.total_len), dtype=np.float32)
        hip_lib().nb_hip_ensemble_potential(self._h, out.ctypes.data)
        return out

    def potential_at(self, points, softening):
        """nb_hip_ensemble_potential_at: Phi of every member at its points -- (n, 2) for all members or (B, n, 2), one set
        per member -- with one softening; float32 (B, n).  Member b's row is bit-identical to SimPipeline.potential_at of
        the same particles.  Ragged ensembles included."""
        return _ensemble_field(hip_lib().nb_hip_ensemble_potential_at, self._h, self.count, 1, softening, points=points)

    def potential_map(self, views, softening):
        """nb_hip_ensemble_potential_map: Phi at every pixel centre, float32 (B, height, width); views: one RenderView for
        all, or one per member."""
        return _ensemble_field(hip_lib().nb_hip_ensemble_potential_map, self._h, self.count, 1, softening, views=views)

    def acceleration_at(self, points, softening):
        """nb_hip_ensemble_acceleration_at: g of every member at its points, float32 (B, n, 2)."""
        return _ensemble_field(hip_lib().nb_hip_ensemble_acceleration_at, self._h, self.count, 2, softening, points=points)

    def acceleration_map(self, views, softening):
        """nb_hip_ensemble_acceleration_map: g at every pixel centre, float32 (B, height, width, 2)."""
        return _ensemble_field(hip_lib().nb_hip_ensemble_acceleration_map, self._h, self.count, 2, softening, views=views)

    def pair_counts(self, edges, classes=("mm",), return_unplaced=False):
        """nb_hip_ensemble_pair_counts, one launch for all members: the pairs of particles per row of separations and per class (include/nbody_paircount.h), uint64
        (B, bins + 2, 3) with the columns (massive-massive, massive-massless, massless-massless); row 0 lies inside edges[0], row
        bins + 1 at or beyond edges[-1].  classes: any subset of "mm", "mt", "tt", or "all"; a class not asked for is zeros and is
        never evaluated.  With return_unplaced also the pairs per class whose squared separation is NaN.  Every count is exact:
        device, host and numpy agree bit for bit.  nb.profile_edges makes edges, nb.pair_curves reads the result."""
        return _pair_counts(hip_lib().nb_hip_ensemble_pair_counts, self._h, self.count, edges, classes, return_unplaced)

    def neighbours(self, radius=None, receivers="all", sources="all"):
        """nb_hip_ensemble_neighbours, one launch for all members: the nearest neighbour of every particle (include/nbody_neighbour.h): (q, index), or (q, index, count)
        when a radius is given -- q float32, the squared distance to the closest other particle of `sources` (+inf without one);
        index uint32, which one (the smallest index among equal q; nb.NB_NEIGH_NONE without one); count uint32, how many lie
        within `radius`.  receivers / sources: "massive", "massless" or "all"; a particle that is no receiver gets
        (+inf, NONE, 0) and a class that is neither is never read.  Device, host and numpy agree bit for bit.
        nb.neighbour_distance and nb.closest_pairs read the result.  Shapes (B, N); a
        ragged ensemble gives lists of per-member arrays, as potential() does.  An index counts within its member."""
        if self.is_ragged:
            return _neighbours(hip_lib().nb_hip_ensemble_neighbours, int(self.offsets[-1]), self.offsets, radius, receivers, sources)(self._h)
        return _neighbours(hip_lib().nb_hip_ensemble_neighbours, self.count * self.total_len, None, radius, receivers, sources,
                           shape=(self.count, self.total_len))(self._h)

    def profile(self, edges, centre=(0.0, 0.0), centre_velocity=(0.0, 0.0), weights="mass", return_unplaced=False):
        """nb_hip_ensemble_profile: the annulus moments of every member (include/nbody_profile.h), float64 (B, bins + 2, 6); the edges are
        shared, centre and centre_velocity are (2,) for all members or (B, 2).  Member b's rows are bit-identical to
        SimPipeline.profile of the same particles; ragged ensembles included.  With return_unplaced also the uint32 (B,) counts of
        particles whose squared radius is NaN."""
        e, bins, c, mode = _profile_args(edges, centre, centre_velocity, weights, self.count)
        out, lost = np.empty((self.count, bins + 2, NB_PROFILE_QTY), dtype=np.float64), np.zeros(self.count, dtype=np.uint32)
        hip_lib().nb_hip_ensemble_profile(self._h, e.ctypes.data, bins, c.ctypes.data, mode, out.ctypes.data, lost.ctypes.data)
        return (out, lost) if return_unplaced else out

    def tidal_at(self, points, softening):
        """nb_hip_ensemble_tidal_at: the tidal tensor of every member at its points, float32 (B, n, 3) in the order (xx, xy,
        yy).  Member b's rows are bit-identical to SimPipeline.tidal_at of the same particles.  Ragged ensembles included."""
        return _ensemble_field(hip_lib().nb_hip_ensemble_tidal_at, self._h, self.count, 3, softening, points=points)

    def tidal_map(self, views, softening):
        """nb_hip_ensemble_tidal_map: the tidal tensor at every pixel centre, float32 (B, height, width, 3)."""
        return _ensemble_field(hip_lib().nb_hip_ensemble_tidal_map, self._h, self.count, 3, softening, views=views)

    def last_diag_ms(self):
        """tuning hook: device ms of the kernels of the last energy() / potential() / potential_at() / potential_map() /
        acceleration_at() / acceleration_map() / tidal_at() / tidal_map() / profile() / pair_counts() / neighbours(); 0.0 after a
        call that had nothing to launch."""
        return float(hip_lib().nb_hip_ensemble_last_diag_ms(self._h))

    def bounds(self):
        """nb_hip_ensemble_bounds: float32 (B, 4), member b's [min.x, min.y, max.x, max.y]."""
        out = np.empty((self.count, 4), dtype=np.float32)
        hip_lib().nb_hip_ensemble_bounds(self._h, out.ctypes.data)
        return out

    def render_counts(self, views):
        """nb_hip_ensemble_render_counts: uint32 (B, 3, height, width); views: one RenderView for all, or one per member."""
        arr, w, h = _view_array(views, self.count)
        out = np.empty((self.count, 3, h, w), dtype=np.uint32)
        hip_lib().nb_hip_ensemble_render_counts(self._h, arr, out.ctypes.data)
        return out

    def render(self, views, palette=None):
        """nb_hip_ensemble_render_rgba: uint8 (B, height, width, 4); palette None = DefaultRenderPalette."""
        arr, w, h = _view_array(views, self.count)
        out = np.empty((self.count, h, w, 4), dtype=np.uint8)
        pal = palette if palette is not None else default_palette()
        hip_lib().nb_hip_ensemble_render_rgba(self._h, arr, C.byref(pal), out.ctypes.data)
        return out

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


class WorldBatch:
    """include/nbody_batch.h WorldBatch, bound 1:1: (B, n, 8) particles in caller order; every member is partitioned
    like CreateWorld partitions it.  WorldBatch.ragged(list of (N_b, 8) arrays) makes a batch whose members differ in size
    (include/nbody_batch_ragged.h): particles() and potential() then return lists of per-member arrays."""

    is_ragged = False

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

    def energy(self):
        """GetWorldBatchEnergy (include/nbody_batch_diag.h): one dict per member, as World.energy() gives it."""
        out = (WorldEnergy * self.count)()
        nbody_lib().GetWorldBatchEnergy(self._h, out)
        return [e.as_dict() for e in out]

    def potential(self):
        """GetWorldBatchPotential: Phi_i of every particle of every member, float32 (B, n), in member(b)'s order."""
        if self.is_ragged:
            flat = np.empty(int(self.offsets[-1]), dtype=np.float32)
            nbody_lib().GetWorldBatchPotential(self._h, flat.ctypes.data)
            return _unpacked(flat, self.offsets)
        out = np.empty((self.count, self.size), dtype=np.float32)
        nbody_lib().GetWorldBatchPotential(self._h, out.ctypes.data)
        return out

    def potential_at(self, points, softening):
        """GetWorldBatchPotentialAt (include/nbody_batch_field.h): Phi of every member at its points -- (n, 2) for all
        members or (B, n, 2) -- float32 (B, n); ragged batches included."""
        return _ensemble_field(nbody_lib().GetWorldBatchPotentialAt, self._h, self.count, 1, softening, points=points)

    def potential_map(self, views, softening):
        """RenderWorldBatchPotential: float32 (B, height, width); views: one RenderView for all, or one per member."""
        return _ensemble_field(nbody_lib().RenderWorldBatchPotential, self._h, self.count, 1, softening, views=views)

    def acceleration_at(self, points, softening):
        """GetWorldBatchAccelerationAt: g of every member at its points, float32 (B, n, 2)."""
        return _ensemble_field(nbody_lib().GetWorldBatchAccelerationAt, self._h, self.count, 2, softening, points=points)

    def acceleration_map(self, views, softening):
        """RenderWorldBatchAcceleration: float32 (B, height, width, 2)."""
        return _ensemble_field(nbody_lib().RenderWorldBatchAcceleration, self._h, self.count, 2, softening, views=views)

    def pair_counts(self, edges, classes=("mm",), return_unplaced=False):
        """GetWorldBatchPairCounts (include/nbody_batch_paircount.h): the pairs of particles per row of separations and per class (include/nbody_paircount.h), uint64
        (B, bins + 2, 3) with the columns (massive-massive, massive-massless, massless-massless); row 0 lies inside edges[0], row
        bins + 1 at or beyond edges[-1].  classes: any subset of "mm", "mt", "tt", or "all"; a class not asked for is zeros and is
        never evaluated.  With return_unplaced also the pairs per class whose squared separation is NaN.  Every count is exact:
        device, host and numpy agree bit for bit.  nb.profile_edges makes edges, nb.pair_curves reads the result."""
        return _pair_counts(nbody_lib().GetWorldBatchPairCounts, self._h, self.count, edges, classes, return_unplaced, spec=True)

    def neighbours(self, radius=None, receivers="all", sources="all"):
        """GetWorldBatchNeighbours (include/nbody_batch_neighbour.h): the nearest neighbour of every particle (include/nbody_neighbour.h): (q, index), or (q, index, count)
        when a radius is given -- q float32, the squared distance to the closest other particle of `sources` (+inf without one);
        index uint32, which one (the smallest index among equal q; nb.NB_NEIGH_NONE without one); count uint32, how many lie
        within `radius`.  receivers / sources: "massive", "massless" or "all"; a particle that is no receiver gets
        (+inf, NONE, 0) and a class that is neither is never read.  Device, host and numpy agree bit for bit.
        nb.neighbour_distance and nb.closest_pairs read the result.  Shapes (B, N), in
        member(b)'s order; a ragged batch gives lists of per-member arrays, as potential() does."""
        if self.is_ragged:
            return _neighbours(nbody_lib().GetWorldBatchNeighbours, int(self.offsets[-1]), self.offsets, radius, receivers, sources, spec=True)(self._h)
        return _neighbours(nbody_lib().GetWorldBatchNeighbours, self.count * self.size, None, radius, receivers, sources, spec=True,
                           shape=(self.count, self.size))(self._h)

    def profile(self, edges, centre=(0.0, 0.0), centre_velocity=(0.0, 0.0), weights="mass", return_unplaced=False):
        """GetWorldBatchProfile (include/nbody_batch_profile.h): the annulus moments of every member (include/nbody_profile.h), float64 (B, bins + 2, 6); the edges are
        shared, centre and centre_velocity are (2,) for all members or (B, 2).  Member b's rows are bit-identical to
        SimPipeline.profile of the same particles; ragged ensembles included.  With return_unplaced also the uint32 (B,) counts of
        particles whose squared radius is NaN."""
        e, bins, c, mode = _profile_args(edges, centre, centre_velocity, weights, self.count)
        out, lost = np.empty((self.count, bins + 2, NB_PROFILE_QTY), dtype=np.float64), np.zeros(self.count, dtype=np.uint32)
        specs = _profile_specs(e, bins, c, mode)
        nbody_lib().GetWorldBatchProfile(self._h, specs, self.count, out.ctypes.data, lost.ctypes.data)
        return (out, lost) if return_unplaced else out

    def tidal_at(self, points, softening):
        """GetWorldBatchTidalAt (include/nbody_batch_tidal.h): the tidal tensor of every member at its points, float32
        (B, n, 3) in the order (xx, xy, yy); ragged batches included."""
        return _ensemble_field(nbody_lib().GetWorldBatchTidalAt, self._h, self.count, 3, softening, points=points)

    def tidal_map(self, views, softening):
        """RenderWorldBatchTidal: float32 (B, height, width, 3)."""
        return _ensemble_field(nbody_lib().RenderWorldBatchTidal, self._h, self.count, 3, softening, views=views)

    def bounds(self):
        """GetWorldBatchBounds (include/nbody_batch_render.h): float32 (B, 4)."""
        out = np.empty((self.count, 4), dtype=np.float32)
        nbody_lib().GetWorldBatchBounds(self._h, out.ctypes.data)
        return out

    def fit_views(self, width, height):
        """FitWorldBatchViews: a list of B RenderViews, each showing every finite particle of its member."""
        arr = (RenderView * self.count)()
        nbody_lib().FitWorldBatchViews(self._h, width, height, arr)
        return [RenderView.from_buffer_copy(v) for v in arr]

    def render_counts(self, views):
        """RenderWorldBatchCounts: uint32 (B, 3, height, width); views: one RenderView for all, or one per member."""
        arr, w, h = _view_array(views, self.count)
        out = np.empty((self.count, 3, h, w), dtype=np.uint32)
        nbody_lib().RenderWorldBatchCounts(self._h, arr, out.ctypes.data)
        return out

    def render(self, views, palette=None):
        """RenderWorldBatch: uint8 (B, height, width, 4); palette None = DefaultRenderPalette."""
        arr, w, h = _view_array(views, self.count)
        out = np.empty((self.count, h, w, 4), dtype=np.uint8)
        nbody_lib().RenderWorldBatch(self._h, arr, C.byref(palette) if palette is not None else None, out.ctypes.data)
        return out


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


class World:
    """include/nbody.h World, bound 1:1 (CreateWorld / UpdateWorld_CPU / UpdateWorld_GPU / ...)."""

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

    def energy(self):
        """GetWorldEnergy (include/nbody_diag.h) as a dict; "total" = kinetic + potential."""
        e = WorldEnergy()
        nbody_lib().GetWorldEnergy(self._h, C.byref(e))
        return e.as_dict()

    def potential(self):
        """GetWorldPotential: Phi_i of every particle (float32, in the order particles() returns them)."""
        out = np.empty(self.size, dtype=np.float32)
        nbody_lib().GetWorldPotential(self._h, out.ctypes.data)
        return out

    def potential_at(self, points, softening):
        """GetWorldPotentialAt (include/nbody_field.h): Phi at the (n, 2) points with one softening, float32 (n,)."""
        pts = as_points(points)
        out = np.empty(pts.shape[0], dtype=np.float32)
        nbody_lib().GetWorldPotentialAt(self._h, pts.ctypes.data, pts.shape[0], softening, out.ctypes.data)
        return out

    def potential_map(self, view, softening):
        """RenderWorldPotential: Phi at every pixel centre of the view, float32 (height, width)."""
        out = np.empty((view.height, view.width), dtype=np.float32)
        nbody_lib().RenderWorldPotential(self._h, C.byref(view), softening, out.ctypes.data)
        return out

    def acceleration_at(self, points, softening):
        """GetWorldAccelerationAt (include/nbody_gravity.h): g at the (n, 2) points with one softening, float32 (n, 2)."""
        pts = as_points(points)
        out = np.empty((pts.shape[0], 2), dtype=np.float32)
        nbody_lib().GetWorldAccelerationAt(self._h, pts.ctypes.data, pts.shape[0], softening, out.ctypes.data)
        return out

    def acceleration_map(self, view, softening):
        """RenderWorldAcceleration: g at every pixel centre of the view, float32 (height, width, 2)."""
        out = np.empty((view.height, view.width, 2), dtype=np.float32)
        nbody_lib().RenderWorldAcceleration(self._h, C.byref(view), softening, out.ctypes.data)
        return out

    def pair_counts(self, edges, classes=("mm",), return_unplaced=False):
        """GetWorldPairCounts: the pairs of particles per row of separations and per class (include/nbody_paircount.h), uint64
        (bins + 2, 3) with the columns (massive-massive, massive-massless, massless-massless); row 0 lies inside edges[0], row
        bins + 1 at or beyond edges[-1].  classes: any subset of "mm", "mt", "tt", or "all"; a class not asked for is zeros and is
        never evaluated.  With return_unplaced also the pairs per class whose squared separation is NaN.  Every count is exact:
        device, host and numpy agree bit for bit.  nb.profile_edges makes edges, nb.pair_curves reads the result."""
        return _pair_counts(nbody_lib().GetWorldPairCounts, self._h, None, edges, classes, return_unplaced, spec=True)

    def neighbours(self, radius=None, receivers="all", sources="all"):
        """GetWorldNeighbours: the nearest neighbour of every particle (include/nbody_neighbour.h): (q, index), or (q, index, count)
        when a radius is given -- q float32, the squared distance to the closest other particle of `sources` (+inf without one);
        index uint32, which one (the smallest index among equal q; nb.NB_NEIGH_NONE without one); count uint32, how many lie
        within `radius`.  receivers / sources: "massive", "massless" or "all"; a particle that is no receiver gets
        (+inf, NONE, 0) and a class that is neither is never read.  Device, host and numpy agree bit for bit.
        nb.neighbour_distance and nb.closest_pairs read the result.  Shapes (N,), in the order particles() returns them."""
        return _neighbours(nbody_lib().GetWorldNeighbours, self.size, None, radius, receivers, sources, spec=True)(self._h)

    def profile(self, edges, centre=(0.0, 0.0), centre_velocity=(0.0, 0.0), weights="mass", return_unplaced=False):
        """GetWorldProfile: the annulus moments about `centre` moving with `centre_velocity` (include/nbody_profile.h), float64
        (bins + 2, 6) with the columns (count, S, I, L, W, K); row 0 lies inside edges[0], row bins + 1 at or beyond edges[-1].
        weights: "mass" (massive particles, weight m) or "number" (all particles, weight 1).  With return_unplaced also the number
        of particles whose squared radius is NaN.  A natural centre: energy()["center_of_mass"] and momentum / mass (vel is used
        as stored, the caveat of include/nbody_diag.h).  nb.profile_curves / nb.lagrangian_radii read the result."""
        e, bins, c, mode = _profile_args(edges, centre, centre_velocity, weights)
        out, lost = np.empty((bins + 2, NB_PROFILE_QTY), dtype=np.float64), np.zeros(1, dtype=np.uint32)
        spec = _profile_specs(e, bins, c[None, :], mode)
        nbody_lib().GetWorldProfile(self._h, spec, out.ctypes.data, lost.ctypes.data)
        return (out, int(lost[0])) if return_unplaced else out

    def tidal_at(self, points, softening):
        """GetWorldTidalAt (include/nbody_tidal.h): the tidal tensor dg/dp at the (n, 2) points with one softening, float32
        (n, 3) in the order (xx, xy, yy)."""
        pts = as_points(points)
        out = np.empty((pts.shape[0], 3), dtype=np.float32)
        nbody_lib().GetWorldTidalAt(self._h, pts.ctypes.data, pts.shape[0], softening, out.ctypes.data)
        return out

    def tidal_map(self, view, softening):
        """RenderWorldTidal: the tidal tensor at every pixel centre of the view, float32 (height, width, 3)."""
        out = np.empty((view.height, view.width, 3), dtype=np.float32)
        nbody_lib().RenderWorldTidal(self._h, C.byref(view), softening, out.ctypes.data)
        return out

    def bounds(self):
        """GetWorldBounds (include/nbody_render.h): float32 [min.x, min.y, max.x, max.y]."""
        out = np.empty(4, dtype=np.float32)
        nbody_lib().GetWorldBounds(self._h, out.ctypes.data)
        return out

    def fit_view(self, width, height):
        """FitWorldView: the RenderView that shows every finite particle on a width x height screen."""
        v = RenderView()
        nbody_lib().FitWorldView(self._h, width, height, C.byref(v))
        return v

    def render_counts(self, view):
        """RenderWorldCounts: uint32 (3, height, width)."""
        out = np.empty((3, view.height, view.width), dtype=np.uint32)
        nbody_lib().RenderWorldCounts(self._h, C.byref(view), out.ctypes.data)
        return out

    def render(self, view, palette=None):
        """RenderWorld: uint8 (height, width, 4); palette None = DefaultRenderPalette."""
        out = np.empty((view.height, view.width, 4), dtype=np.uint8)
        nbody_lib().RenderWorld(self._h, C.byref(view), C.byref(palette) if palette is not None else None, out.ctypes.data)
        return out


_cpu_best = None


def cpu_best_lib():
    """libnbody_cpu_best.so (csrc/cpu_best.c): the informational CPU variants of sim_cpu.c; never behind UpdateWorld_CPU."""
    global _cpu_best
    if _cpu_best is None:
        path = os.path.join(LIB_DIR, "libnbody_cpu_best.so")
        _build_if_missing(path)
        lib = C.CDLL(path)
        lib.nb_cpu_variant_count.restype = C.c_int
        lib.nb_cpu_variant_name.restype = C.c_char_p
        lib.nb_cpu_variant_name.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
        lib.nb_cpu_variant_update.restype = C.c_int
        lib.nb_cpu_variant_update.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32]
        _cpu_best = lib
    return _cpu_best


def cpu_variants():
    """[(isa, runs on this CPU, description)] of the informational CPU steppers."""
    lib, out = cpu_best_lib(), []
    for i in range(lib.nb_cpu_variant_count()):
        ok, what = C.c_int(0), C.c_char_p()
        name = lib.nb_cpu_variant_name(i, C.byref(ok), C.byref(what))
        out.append((name.decode(), bool(ok.value), what.value.decode()))
    return out


def cpu_variant_update(isa, particles, mass_len, dt, n=1):
    """n Jacobi steps of a PARTITIONED array (sources first) with one informational CPU variant; returns the new array."""
    a = as_particles(particles).copy()
    if cpu_best_lib().nb_cpu_variant_update(isa.encode(), a.ctypes.data, a.shape[0], mass_len, dt, n) != 0:
        raise RuntimeError(f"CPU variant {isa!r} is unknown or not supported by this CPU")
    return a


def make_galaxies(particle_count, galaxy_count, seed=None, own_rng=False):
    """include/galaxy.h MakeGalaxies; `seed` calls libc srand first (bench.c:42 uses 11037).
    own_rng=True: MakeGalaxiesSeeded, the libc-independent stream (seed required)."""
    L = nbody_lib()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    if own_rng:
        p = L.MakeGalaxiesSeeded(particle_count, galaxy_count, int(seed))
    else:
        if seed is not None:
            libc.srand(C.c_uint(seed))
        p = L.MakeGalaxies(particle_count, galaxy_count)
    a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(particle_count, 8)).copy()
    libc.free(p)
    return a
