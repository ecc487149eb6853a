"""nbody_amd -- Python view of the MI355X-native N-body engine (for tests, bench.py and tooling).

The product is C: `lib/libnbody_hip.so` (HIP kernels + the C-ABI of include/nbody_hip.h) and
`lib/libnbody.so` (the include/nbody.h / galaxy.h surface, C host code).  This package only binds
them with ctypes; no arithmetic happens in Python and there is no fallback: if the libraries are
missing, importing the bound functions raises, and any GPU call without a gfx950 device aborts
inside the library (reference error convention, src/lib/util.h:17-29).

Particles travel as float32 arrays of shape (n, 8): pos.xy vel.xy acc.xy mass radius --
byte-identical to `Particle[n]` (include/nbody.h).

_abi the structures, tables and loaders; device what concerns no world; reads the read-only calls, written once; pipeline, batch
and world the four classes that inherit them; analysis the numpy readers of their results; host the CPU variants and the galaxy
generator.  Everything public is reachable from here.
"""
import ctypes as C    # noqa: F401  callers spell ctypes types nb.C.c_double
import os             # noqa: F401  os and np have always been reachable through the package
import numpy as np    # noqa: F401

from ._abi import (ALLGATHER_FN, CLOCK_SAMPLER_MAX_MS, HIP_API, HIP_SO, LIB_DIR, NB_ADAPT_CONTINUE, NB_ADAPT_LEAPFROG,  # noqa: F401
                   NB_ADAPT_PRIME, NB_G, NB_GROUP_NONE, NB_NEIGH_ALL, NB_NEIGH_MASSIVE, NB_NEIGH_MASSLESS, NB_NEIGH_NONE, NB_PAIRS_ALL,
                   NB_PAIRS_COLUMNS, NB_PAIRS_MAX_BINS, NB_PAIRS_MM, NB_PAIRS_MT, NB_PAIRS_TABLE, NB_PAIRS_TT, NB_PROFILE_BY_MASS,
                   NB_PROFILE_BY_NUMBER, NB_PROFILE_CHUNK, NB_PROFILE_MAX_BINS, NB_PROFILE_QTY, NBODY_API, NBODY_SO, PKG_DIR,
                   PUBLIC_KNOBS, ROOT, TUNE_API, UNIQUE_ID_BYTES, NbAdaptive, NbAdaptiveResult, NbShardPlan, RenderPalette,
                   RenderView, WorldData, WorldEnergy, WorldGroupSpec, WorldNeighbourSpec, WorldPairSpec, WorldProfileSpec, adaptive_cfg,
                   as_ensemble, as_particles, as_points, default_palette, energy_row, hip_lib, nbody_lib)
from .analysis import (closest_pairs, contact_sheet, group_members, group_table, lagrangian_radii, linking_length_for,  # noqa: F401
                       neighbour_distance, pair_curves, profile_curves, profile_edges, tidal_invariants)
from .batch import SimBatch, trace_rows  # noqa: F401
from .device import (clock_sampler_begin, clock_sampler_end, comm_unique_id, deal_item, device_count, device_info,  # noqa: F401
                     hip_error_string, live_resources, plan_deal, plan_launch, preflight_ipc_export, preflight_ipc_open,
                     preflight_peers, probe_clock, shard_plan)
from .host import cpu_best_lib, cpu_variant_update, cpu_variants, make_galaxies  # noqa: F401
from .pipeline import LocalShardGroup, SimPipeline  # noqa: F401
from .world import World, WorldBatch  # noqa: F401
