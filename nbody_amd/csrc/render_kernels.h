// render_kernels.h -- what render.hip (a SimPipeline's render calls) and batch_observe.hip (a SimBatch's) need of
// render_kernels.hip: the launchers of every render kernel, for a world and for an ensemble.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "nbody_render.h"

namespace nb {
namespace render {

// One workgroup's LDS budget for the three class planes of a tile: 3 * width * height * 4 bytes up to here run on the tile
// path (a 64 x 64 thumbnail; with the 12 KiB disc list two workgroups fit a compute unit's 160 KiB), larger tiles on the
// global path.  Up to here the tile path is ahead (profiles/r10_batch_render_probe.json: 0.020 against 0.043 ms of kernels for
// 256 frames of N = 3 000 at 64 x 64); no measurement above it, so it is not raised.
constexpr uint32_t TILE_LDS_BYTES = 48u * 1024u;

// One item of a disc list in device memory: a world's, or the one list of an ensemble's global path, where the member the
// disc belongs to rides above the class.  A world writes member 0.
struct Disc {
    float sx, sy, rho;
    uint32_t cls_member;   // cls | member << 2
};

// The SoA arrays of a SimBatch (member b's rows start at b * stride; only rows [0, n) exist) and the views of one call.
struct EnsembleRenderParams {
    const float2 *pos;         // pos[cur]: the latest state
    const float *mass;
    const float *radius;
    uint32_t n;                // particles per member
    uint32_t stride;           // rows per member (a multiple of 64)
    uint32_t count;            // members
    uint32_t width, height;    // of every view
    const RenderView *views;   // [count], on the device
};

inline bool tile_fits(uint32_t width, uint32_t height) {
    return (uint64_t)width * height * NB_RENDER_CLASSES * sizeof(uint32_t) <= TILE_LDS_BYTES;
}

// words of the global path's count buffer: the images and, behind them, the disc cursor (one clear covers both)
inline size_t global_count_words(uint32_t count, uint32_t width, uint32_t height) {
    return (size_t)count * NB_RENDER_CLASSES * width * height + 1;
}

// ---- a world: n particles from row 0 ------------------------------------------------------------------------------------

// keys[0..3] = min key of x, of y, max key of x, of y; set to the identities by the caller in stream order
void launch_bounds(hipStream_t stream, const float2 *pos, uint32_t n, uint32_t *keys);
// Points into counts[3][h][w] (cleared by the caller, like *ndisc), discs that can touch the image onto discs[0 .. *ndisc);
// merge: same-word lanes are merged before they add (the shipped build), else one atomic per lane
void launch_splat(hipStream_t stream, const float2 *pos, const float *mass, const float *radius, uint32_t n, const RenderView &view,
                  bool merge, uint32_t *counts, Disc *discs, uint32_t *ndisc);
// discs[0 .. *ndisc) into counts[3][h][w]; *ndisc is read on the device
void launch_discs(hipStream_t stream, const Disc *discs, const uint32_t *ndisc, uint32_t width, uint32_t height, uint32_t *counts);
// rgba[h][w] from counts[3][h][w]
void launch_shade(hipStream_t stream, const uint32_t *counts, uint32_t plane, const RenderPalette &palette, uint32_t *rgba);

// ---- an ensemble --------------------------------------------------------------------------------------------------------

// keys[b][4] = member b's ordered min / max keys; one workgroup per member, plain stores
void launch_ensemble_bounds(hipStream_t stream, const float2 *pos, uint32_t n, uint32_t stride, uint32_t count, uint32_t *keys);
// The tile path, one launch: counts[count][3][h][w] when palette is NULL, else rgba[count][h][w] (packed) and no count image.
void launch_ensemble_tile(hipStream_t stream, const EnsembleRenderParams &p, uint32_t *counts, const RenderPalette *palette,
                          uint32_t *rgba);
// The global path's splat and disc pass into counts (global_count_words of them, cleared by the caller in stream order;
// discs holds count * n items): two launches.
void launch_ensemble_global(hipStream_t stream, const EnsembleRenderParams &p, uint32_t *counts, Disc *discs);
// rgba[count][h][w] from counts[count][3][h][w]
void launch_ensemble_shade(hipStream_t stream, const uint32_t *counts, uint32_t count, uint32_t plane, const RenderPalette &palette,
                           uint32_t *rgba);

}  // namespace render
}  // namespace nb
