// field.hip -- two fields of the state a pipeline holds at points that are not particles: probes the caller chooses and the
// pixel centres of a view.  The potential (include/nbody_field.h; nb_hip_potential_at / nb_hip_potential_map) and the
// acceleration (include/nbody_gravity.h; nb_hip_acceleration_at / nb_hip_acceleration_map) are one sampler with two pair
// statements.
//
// Definitions (also in the two headers and DESIGN.md section 3): for a sample p and a softening s, with G*m_j = src_gm[j],
// M = mass_len and d_j = x_j - p,
//     Phi(p; s) = - sum_{j < M} G*m_j / sqrt(|d_j|^2 + s)          = diagnostics.hip's Phi_i of a massless receiver at p
//     g(p; s)   =   sum_{j < M} G*m_j d_j / (|d_j|^2 + s)^(3/2)    = what a step stores in acc[] for such a receiver
// both with radius s.  A sample is never a source, so no term is excluded: Phi runs the unmasked pair statement only, and a
// sample exactly on a source gets d_j = 0 over a finite denominator in g, a zero term.
//
// What differs between the two is the quantity policy Q (Potential, Acceleration): the pair statement behind one block of
// sources (diag_common.h's unmasked pair; interaction_asm.h's NB_INTERACTION2_ASM), the number of components and the store.
// The policies, Params, load_samples, store_sample and slice_sum live in field_kernels.h, which the sampler of an ensemble
// (batch_field.hip) shares.  The summation is written once, and it is diag_common.h's: fp32 sums
// from 0.0f over a block of 256 sources with j ascending, float64 totals per block, and the eight source slices
// [w * per, (w + 1) * per), per = ceil(ceil(M / 256) / 8), added in wave order from 0.0, each component rounded once to
// float32.  A result is defined by that order, not by which wave adds what, so the two kernels give the same bits
// (and Phi the bits potential_kernel gives a massless particle of radius s at the same place):
//   sample_split_kernel  potential_kernel's shape: the 8 waves of a workgroup share one tile of 128 samples (64 lanes x 2)
//                        and each walks 1/8 of the source blocks; the slices meet in part[C][W][TILE] (LDS, float64).
//                        For large M.
//   sample_wave_kernel   ensemble_phi_kernel's shape: every wave owns a tile and walks the eight slices itself.  No LDS, no
//                        barrier.  For small worlds under large images, where the split's workgroups are mostly waves
//                        without a block (7 of 8 at M <= 256) and the tiles alone fill the chip.
// Both kernels, and the pick_wave_shape() that chooses between them in one place, are in field_sampler.h: tidal.hip builds
// the same sampler for a third policy.  Sources stay on the scalar-cache route in both (wave-uniform,
// s_load_dwordx16 / x8, 8 per fetch, single sources for a ragged end).  MAP = true: a lane forms its two samples from the
// view's column and row coordinates (sample i = py * width + px reads xs[px] and ys[py]; the host computed both arrays,
// render_common.h); MAP = false: it loads them.  A sample with a non-finite coordinate stores NaN in every component.  No
// atomics; vector stores only, one per sample.
#include "pipeline_internal.h"
#include "diag_common.h"
#include "field_common.h"
#include "field_kernels.h"
#include "interaction_asm.h"
#include "nbody_hip_tuning.h"
// sample_split_kernel, sample_wave_kernel, pick_wave_shape() and the host side of a call (sample_at, sample_map): shared with
// tidal.hip, which instantiates the same sampler for the third quantity
#include "field_sampler.h"

extern "C" {

void nb_hip_potential_at(SimPipeline *s, const float *points, uint32_t n, float softening, float *phi) {
    sample_at<fd::Potential>(s, "nb_hip_potential_at", points, n, softening, phi);
}

void nb_hip_potential_map(SimPipeline *s, const RenderView *view, float softening, float *phi) {
    sample_map<fd::Potential>(s, "nb_hip_potential_map", view, softening, phi);
}

void nb_hip_acceleration_at(SimPipeline *s, const float *points, uint32_t n, float softening, float *acc) {
    sample_at<fd::Acceleration>(s, "nb_hip_acceleration_at", points, n, softening, reinterpret_cast<float2 *>(acc));
}

void nb_hip_acceleration_map(SimPipeline *s, const RenderView *view, float softening, float *acc) {
    sample_map<fd::Acceleration>(s, "nb_hip_acceleration_map", view, softening, reinterpret_cast<float2 *>(acc));
}

}  // extern "C"
