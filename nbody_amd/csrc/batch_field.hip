// batch_field.hip -- the potential and the acceleration field of EVERY member of an ensemble (SimBatch) at probe points and
// over views, in one launch (include/nbody_hip.h nb_hip_ensemble_potential_at / _potential_map / _acceleration_at /
// _acceleration_map; the entry points sit in batch_observe.hip).
//
// The definitions, the two pair statements and the summation are field.hip's, through field_kernels.h: member b's values
// are, bit for bit, what nb_hip_potential_at / _map / nb_hip_acceleration_at / _map give the same particles alone in a
// SimPipeline, on either of its kernel shapes, because a result is defined by a summation order and not by which wave adds
// what.  ensemble_sample_kernel is sample_wave_kernel with blockIdx.y = member: up to 4 waves per workgroup, each owning one
// tile of 128 of its member's samples (64 lanes x 2) and walking that member's eight source slices itself (slice_sum).  The
// member's sources are found the one way the device finds a member, uniform or ragged (batch_diag.hip): its rows start at
// member * stride and it has mass_len[member] of them, read from the device with a scalar load; they stay on the scalar-cache
// route (s_load_dwordx16 / x8, wave-uniform; a member's rows start 256-byte aligned because stride is a multiple of 64 rows).
// Every member has the same number of samples n: probes at in + member * 2n, a map's column and row coordinates at in +
// member * (width + height), results at out + member * n.  A wave whose tile lies beyond n leaves at once.  No LDS, no
// barrier, no atomics; vector stores only, one per sample.
//
// One shape only: a member has at most 3 000 sources, 12 blocks of 256, and there are `count` members to fill the chip
// with.  field.hip's split shape wins from 4 blocks up under very large maps only (pick_wave_shape there); that corner is
// priced by tools/batch_field_probe.py, not built.
#include "batch_field.h"
#include "field_kernels.h"

// ensemble_sample_kernel and its launcher: shared with tidal.hip, which instantiates them for the third quantity
#include "ensemble_sampler.h"

namespace nb {
namespace field {

void launch_ensemble_sample(hipStream_t stream, const EnsembleParams &p, uint32_t count, bool acceleration, bool map) {
    if (acceleration)
        launch<Acceleration>(stream, p, count, map);
    else
        launch<Potential>(stream, p, count, map);
}

}  // namespace field
}  // namespace nb
