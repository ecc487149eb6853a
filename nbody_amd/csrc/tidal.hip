// tidal.hip -- the tidal tensor of the state a pipeline or an ensemble holds, at probe points and at the pixel centres of a
// view (include/nbody_tidal.h, include/nbody_batch_tidal.h; nb_hip_tidal_at / nb_hip_tidal_map and the kernels behind
// nb_hip_ensemble_tidal_at / nb_hip_ensemble_tidal_map, whose entry points sit in batch_observe.hip with the ensemble's other
// field calls).  The field sampler's third quantity: for a sample p and a softening s, with G*m_j = src_gm[j], M = mass_len,
// d_j = x_j - p, q_j = |d_j|^2 + s and u_j = q_j^(-1/2),
//     T_ab(p; s) = dg_a/dp_b = sum_{j < M} G*m_j (3 d_a d_b u_j^5 - delta_ab u_j^3)          (xx, xy, yy)
// No term is excluded; a sample exactly on a source gets the finite term diag(-G*m s^(-3/2)).
//
// Nothing here but instantiations.  The pair statement and the float64 finish are field_kernels.h's Tidal policy; the two
// kernel shapes of a pipeline, the rule that picks one ("tidal_shape", the one pick_wave_shape) and the host side of a call
// are field_sampler.h's; the kernel of an ensemble is ensemble_sampler.h's.  So the summation is the sampler's (fp32 sums from
// 0.0f over blocks of 256 sources, float64 block totals, eight slices added in wave order) for each of the four running
// sums, a result is defined by that order, and all six kernels of this file give a sample the same bits.
//
// Registers: the kernels hold four running sums where g holds two; the one-wave-per-tile shapes keep two sets of float64
// sums (the slice's and the sample's).  They are built for eight waves per SIMD (at most 64 VGPRs) without scratch, which
// tests/test_tidal_cpu.py reads off the compiled code.
#include "pipeline_internal.h"
#include "diag_common.h"
#include "field_common.h"
#include "field_kernels.h"
#include "nbody_hip_tuning.h"
#include "field_sampler.h"
#include "ensemble_sampler.h"

namespace nb {
namespace field {

void launch_ensemble_tidal(hipStream_t stream, const EnsembleParams &p, uint32_t count, bool map) {
    launch<Tidal>(stream, p, count, map);
}

}  // namespace field
}  // namespace nb

extern "C" {

void nb_hip_tidal_at(SimPipeline *s, const float *points, uint32_t n, float softening, float *t) {
    sample_at<fd::Tidal>(s, "nb_hip_tidal_at", points, n, softening, reinterpret_cast<fd::Tidal::Out *>(t));
}

void nb_hip_tidal_map(SimPipeline *s, const RenderView *view, float softening, float *t) {
    sample_map<fd::Tidal>(s, "nb_hip_tidal_map", view, softening, reinterpret_cast<fd::Tidal::Out *>(t));
}

}  // extern "C"
