"""The C ABI as ctypes sees it: the structures and constants of include/*.h, one table of (restype, argtypes) per library, the
loaders, and the checks that turn arrays into what the ABI takes.  Imports nothing from its siblings but build, and that only
when a library is missing."""
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


NB_GROUP_NONE = 0xFFFFFFFF     # include/nbody_group.h


class WorldGroupSpec(C.Structure):
    """include/nbody_group.h WorldGroupSpec."""
    _fields_ = [("members", C.c_uint32), ("linking_length", C.c_float)]


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
    "nb_hip_groups": (None, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
    "nb_hip_ensemble_groups": (None, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
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
    "nb_hip_group_span": (C.c_uint32, [C.c_uint32]),
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
# include/nbody_neighbour.h + include/nbody_batch_neighbour.h + include/nbody_group.h + include/nbody_batch_group.h
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
    # include/nbody_group.h, include/nbody_batch_group.h
    "GetWorldGroups": (None, [C.c_void_p, C.POINTER(WorldGroupSpec), C.c_void_p, C.c_void_p]),
    "GetWorldBatchGroups": (None, [C.c_void_p, C.POINTER(WorldGroupSpec), C.c_void_p, C.c_void_p]),
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


def as_ensemble(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 8:
        raise ValueError("an ensemble must have shape (members, n, 8)")
    return a
