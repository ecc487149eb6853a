// batch_diag.hip -- energy, momentum and per-particle potential of every member of an ensemble (SimBatch), in one pass
// over all members (include/nbody_hip.h nb_hip_ensemble_energy / nb_hip_ensemble_potential; the entry points sit in
// batch_observe.hip).
//
// The definitions and the arithmetic are those of diagnostics.hip, through diag_common.h: member b's result is, bit for
// bit, what nb_hip_energy / nb_hip_potential give for the same particles alone in a SimPipeline.  That is possible because
// a result is defined by a summation order, not by which wave adds what (diag_common.h).
//
// potential_kernel is the wrong shape for small worlds: its 8 waves slice the sources in blocks of 256, so a member with
// M <= 256 would leave 7 of 8 waves idle.  ensemble_phi_kernel turns the mapping round: gridDim.y = member, every WAVE
// owns one tile of 128 receivers (64 lanes x 2) and walks its member's whole source list itself, in the order the eight
// waves of potential_kernel would: for w = 0..7 the blocks [w * per, (w + 1) * per) into a float64 s_w from 0.0, then
// 0.0 + s_0 + ... + s_7, all in registers.  Sources stay on the scalar-cache route (s_load_dwordx16 / x8, wave-uniform;
// a member's rows start 256-byte aligned because stride is a multiple of 64 rows); only the sources that are the wave's own
// 128 receivers run the masked body (a block is cut there: a member of 250 has ONE block, which potential_kernel would
// mask whole).  No LDS, no barrier: a workgroup is just 1..4 such waves of one member, and a wave whose
// tile lies beyond the member's receivers leaves at once.
// With `slab`, the wave reduces its tile's eight float64 terms in the tree of potential_kernel -- rows t and t + half for
// half = 64, 32, .. 1, dead lanes 0 -- where the first level adds the lane's own two receivers and the other six move
// through the cross-lane network; lane 0 stores the row.  ensemble_reduce_kernel, one workgroup per member, then adds the
// member's ceil(M_b / 128) rows exactly as energy_reduce_kernel does.  No float atomics, vector stores only.
//
// A RAGGED ensemble (members of different N) needs nothing new for its energy sums: they run over a member's mass_len[b]
// massive receivers, read from the device already, and the slab rows only have to be sized by the largest member.  Its
// potential runs over ALL of a member's particles and is stored packed, so the receiver count and the output offset are per
// member: ensemble_phi_kernel<RaggedDiagParams> reads both from device arrays and is otherwise the same statements, so
// member b's values are the bits nb_hip_ensemble_potential gives the same particles in a uniform ensemble.
#include "batch_diag.h"
#include "diag_common.h"

#include <type_traits>

namespace nbd {
namespace {

constexpr int WAVES_MAX = 4;   // tiles (waves) per workgroup

template <typename T>
__device__ __forceinline__ T uniform_load(const T *p) {   // wave-uniform address, read-only for the launch: s_load
    return *(const T __attribute__((address_space(4))) *)(uintptr_t)p;
}

// One body for both ways of addressing the members (batch_diag.h; the step kernels' member_of, kernels.hip, mirrored).
// What depends on it is how many receivers member b has in this launch and where its potentials start in p.phi: by block
// index p.n and b * p.n, by list (LISTED) both read from the device.  LISTED computes the potential only: nothing of the
// slab is compiled into it.  (The two answers are spelled in the body, not in functions of p: a reference to the
// by-value kernel argument costs the stores of the slab rows their global address space.)
template <class P>
__global__ __launch_bounds__(WAVE * WAVES_MAX) void ensemble_phi_kernel(const P p) {
    constexpr bool LISTED = std::is_same_v<P, RaggedDiagParams>;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t member = blockIdx.y;
    const uint32_t tile = blockIdx.x * p.waves + wid;
    const uint32_t n_src = uniform_load(p.mass_len + member);
    uint32_t n_recv;
    if constexpr (LISTED)
        n_recv = uniform_load(p.n_len + member);
    else
        n_recv = p.slab ? n_src : p.n;   // the energy sums run over the massive receivers only
    const uint32_t rb = tile * TILE;                // first receiver of this wave's tile, member-local
    if (rb >= n_recv) return;
    const size_t base = (size_t)member * p.stride;
    const float2 *pos = p.pos + base;

    float px[K], py[K], r[K];
    uint32_t ri[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        uint32_t i = rb + k * WAVE + lane;
        i = i < n_recv ? i : n_recv - 1;  // tail lanes redo the last receiver; their results are dropped
        const float2 q = pos[i];
        px[k] = q.x;
        py[k] = q.y;
        r[k] = p.radius[base + i];
        ri[k] = i;
    }

    // the eight source slices of potential_kernel's waves, one after another, in whole blocks (diag_common.h)
    double sum[K];
    tile_potential(sum, px, py, r, ri, rb, n_src, ScalarSources{(ConstF)(uintptr_t)pos, (ConstF)(uintptr_t)(p.gm + base)});

    // Phi_i = -sum; the eight terms of the lane's two receivers (tile rows lane and lane + 64)
    size_t packed_at = 0;
    if constexpr (LISTED) packed_at = uniform_load(p.offsets + member);
    double e[K][QTY];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double phi = -sum[k];
        const uint32_t i = rb + k * WAVE + lane;
        const bool live = i < n_recv;
        if (live && (LISTED || p.phi)) p.phi[(LISTED ? packed_at : (size_t)member * p.n) + i] = (float)phi;
        if constexpr (!LISTED)
            if (p.slab) energy_terms(e[k], live, phi, p.mass + base, pos, p.vel + base, i);
    }
    if constexpr (!LISTED) {
        if (!p.slab) return;
        // potential_kernel's tree over the 128 rows of the tile: half = 64 is rows lane and lane + 64, the rest crosses lanes
        double t[QTY];
        tile_tree(t, e);
        if (lane == 0) {
            double *row = p.slab + ((size_t)member * p.tiles + tile) * QTY;
#pragma unroll
            for (int q = 0; q < QTY; q++) row[q] = t[q];
        }
    }
}

// One workgroup per member: member b's ceil(M_b / 128) rows -> out[b][QTY] (reduce_rows, diag_common.h).  M_b = 0: no
// row is read and every sum is 0.
__global__ __launch_bounds__(REDUCE_THREADS) void ensemble_reduce_kernel(const double *slab, const uint32_t *mass_len, uint32_t tiles,
                                                                         double *out) {
    const uint32_t member = blockIdx.x;
    const uint32_t rows = (uniform_load(mass_len + member) + TILE - 1) / TILE;
    reduce_rows(slab + (size_t)member * tiles * QTY, rows, out + (size_t)member * QTY);
}

}  // namespace

uint32_t ensemble_tiles(uint32_t n) { return (n + TILE - 1) / TILE; }

void launch_ensemble_potential(hipStream_t stream, EnsembleDiagParams p, uint32_t count, const uint32_t *n_len, const uint64_t *offsets) {
    p.tiles = ensemble_tiles(p.n);
    p.waves = p.tiles < (uint32_t)WAVES_MAX ? p.tiles : (uint32_t)WAVES_MAX;
    const dim3 grid((p.tiles + p.waves - 1) / p.waves, count);
    if (n_len) {
        const RaggedDiagParams rp = {p, n_len, offsets};
        hipLaunchKernelGGL(ensemble_phi_kernel<RaggedDiagParams>, grid, dim3(WAVE * p.waves), 0, stream, rp);
    } else {
        hipLaunchKernelGGL(ensemble_phi_kernel<EnsembleDiagParams>, grid, dim3(WAVE * p.waves), 0, stream, p);
    }
}

void launch_ensemble_reduce(hipStream_t stream, const double *slab, const uint32_t *mass_len, uint32_t tiles, uint32_t count,
                            double *out) {
    hipLaunchKernelGGL(ensemble_reduce_kernel, dim3(count), dim3(REDUCE_THREADS), 0, stream, slab, mass_len, tiles, out);
}

}  // namespace nbd
