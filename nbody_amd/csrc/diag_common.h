// diag_common.h -- the arithmetic of the energy / potential diagnostics, written once for the two translation units that
// run it on the device: diagnostics.hip (one pipeline: potential_kernel slices the SOURCES over the 8 waves of a
// workgroup) and batch_diag.hip (an ensemble: every wave owns its receivers and walks its member's whole source list).
// Both must give the same bits for the same world (include/nbody_hip.h "World ensembles"), so what defines a result
// lives here and nowhere else:
//   * the pair statement and the fp32 sum over one block of 256 sources, j ascending (pair, group8, block_sum);
//   * one wave's walk over its world's sources for a tile of 128 receivers (tile_potential) and the tile's tree (tile_tree);
//   * the eight float64 terms of one receiver (energy_terms);
//   * the sum of the per-tile rows of one world (reduce_rows, reduce_rows_shfl).
// kernels.hip's traced chain (batch_trace_chain_kernel) runs the same functions on the state it holds in LDS.
// What differs between the two kernels is only which wave adds which block; the ORDER of the float64 additions is the
// same in both: blocks [w * per, (w + 1) * per) from 0.0 for w = 0..7, per = ceil(ceil(M / 256) / 8), then
// 0.0 + s_0 + ... + s_7.  -ffp-contract=off keeps the float64 expressions as written.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "diag_sums.h"

namespace nbd {

constexpr int WAVE = 64;
constexpr int K = 2;                // receivers per lane
constexpr int W = 8;                // source slices of the float64 sum (potential_kernel: one wave each)
constexpr int TILE = WAVE * K;      // receivers per tile
constexpr int BLOCK = 256;          // sources per plain fp32 block sum
constexpr int QTY = NB_DIAG_SUMS;   // float64 quantities per tile row of an energy slab (diag_sums.h)
constexpr int REDUCE_THREADS = 256;

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v8f __attribute__((ext_vector_type(8)));
typedef const float __attribute__((address_space(4))) *ConstF;  // read-only for the whole launch: scalar loads

template <typename V>
__device__ __forceinline__ V cload(ConstF p) {
    return *(const V __attribute__((address_space(4))) *)p;
}

// One source (wave-uniform, SGPRs) against the K receivers of this lane, as one asm statement per pair (as in
// kernels.hip, and for the same reasons: left to hipcc, the two receivers' FMAs become v_pk_fma_f32, which this project
// measured slower beside a transcendental, and the schedule drifts with unrelated edits):
//     v_sub_f32   dx  = sx - x
//     v_sub_f32   dy  = sy - y
//     v_fma_f32   q   = dx * dx + radius      softening: + radius of the RECEIVER, not squared
//     v_fmac_f32  q  += dy * dy
//     v_rsq_f32   q   = 1 / sqrt(q)          at raised wave priority, like the step kernels' rsq
//     v_fmac_f32  phi += (G*m) * q           (the s_setprio 0 before it is the wait state a transcendental's reader needs)
// MASK (the diagonal block only): source j may be receiver i itself; that term is dropped by a select AFTER the rsq
// (r_i = 0 makes it inf, and 0 * inf is NaN), so the masked statement stops at the rsq.
#define NB_PHI_HEAD_ASM                     \
    "v_sub_f32 %[dx], %[sx], %[px]\n\t"     \
    "v_sub_f32 %[dy], %[sy], %[py]\n\t"     \
    "v_fma_f32 %[q], %[dx], %[dx], %[r]\n\t" \
    "v_fmac_f32 %[q], %[dy], %[dy]\n\t"     \
    "s_setprio 3\n\t"                      \
    "v_rsq_f32 %[q], %[q]\n\t"              \
    "s_setprio 0"
// SGPR = false: the same statement with the source in VGPRs that hold a wave-uniform value (a broadcast LDS read: the
// traced chain of kernels.hip records from the positions it keeps in LDS).  Only the operand class differs: the
// instructions, their order and so the bits are the same.
#define NB_PHI_PAIR(SRC)                                                                                      \
    if constexpr (MASK) {                                                                                     \
        asm(NB_PHI_HEAD_ASM                                                                                   \
            : [dx] "=&v"(dx), [dy] "=&v"(dy), [q] "=&v"(q)                                                    \
            : [sx] SRC(sx), [sy] SRC(sy), [px] "v"(px[k]), [py] "v"(py[k]), [r] "v"(r[k]));                   \
        const float n = __builtin_fmaf(g, q, a[k]);                                                           \
        a[k] = j != ri[k] ? n : a[k];                                                                         \
    } else {                                                                                                  \
        asm(NB_PHI_HEAD_ASM "\n\t"                                                                            \
            "v_fmac_f32 %[a], %[g], %[q]"                                                                     \
            : [a] "+v"(a[k]), [dx] "=&v"(dx), [dy] "=&v"(dy), [q] "=&v"(q)                                    \
            : [sx] SRC(sx), [sy] SRC(sy), [g] SRC(g), [px] "v"(px[k]), [py] "v"(py[k]), [r] "v"(r[k]));       \
    }
template <bool MASK, bool SGPR = true>
__device__ __forceinline__ void pair(float (&a)[K], const float (&px)[K], const float (&py)[K], const float (&r)[K],
                                     const uint32_t (&ri)[K], float sx, float sy, float g, uint32_t j) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        float dx, dy, q;
        if constexpr (SGPR) {
            NB_PHI_PAIR("s")
        } else {
            NB_PHI_PAIR("v")
        }
    }
}
#undef NB_PHI_PAIR

template <bool MASK, bool SGPR = true>
__device__ __forceinline__ void group8(float (&a)[K], const float (&px)[K], const float (&py)[K], const float (&r)[K],
                                       const uint32_t (&ri)[K], const v16f &P, const v8f &G, uint32_t j) {
#pragma unroll
    for (int u = 0; u < 8; u++) pair<MASK, SGPR>(a, px, py, r, ri, P[2 * u], P[2 * u + 1], G[u], j + u);
}

// Sources [j0, j1) of one block (j0 a multiple of 256) added to a[]: 8 per scalar fetch (s_load_dwordx16 for the
// positions, s_load_dwordx8 for G*m), then single sources for a ragged end.  One register set, no double buffering: the
// kernel needs ~70 % of the step kernel's issue cycles per pair, and eight waves per SIMD hide the fetch of the next set
// (the step kernel's two alternating sets cost the SGPRs that this kernel's operands need: they spilled to VGPR lanes).
template <bool MASK>
__device__ __forceinline__ void block_sum(float (&a)[K], const float (&px)[K], const float (&py)[K], const float (&r)[K],
                                          const uint32_t (&ri)[K], ConstF sp, ConstF sg, uint32_t j0, uint32_t j1) {
    uint32_t j = j0;
    for (; j + 8 <= j1; j += 8) {
        const v16f P = cload<v16f>(sp + 2 * (size_t)j);
        const v8f G = cload<v8f>(sg + j);
        group8<MASK>(a, px, py, r, ri, P, G, j);
    }
    for (; j < j1; j++) pair<MASK>(a, px, py, r, ri, sp[2 * (size_t)j], sp[2 * (size_t)j + 1], sg[j], j);
}

// The same block with the sources in LDS (positions (x, y) interleaved at sp, G*m at sg, both 16-byte aligned): every
// lane reads the same address, so a group of 8 arrives by broadcast reads in VGPRs.  Same pairs, same order.
template <bool MASK>
__device__ __forceinline__ void block_sum_lds(float (&a)[K], const float (&px)[K], const float (&py)[K], const float (&r)[K],
                                              const uint32_t (&ri)[K], const float *sp, const float *sg, uint32_t j0, uint32_t j1) {
    uint32_t j = j0;
    for (; j + 8 <= j1; j += 8) {
        const v16f P = *reinterpret_cast<const v16f *>(sp + 2 * j);
        const v8f G = *reinterpret_cast<const v8f *>(sg + j);
        group8<MASK, false>(a, px, py, r, ri, P, G, j);
    }
    for (; j < j1; j++) pair<MASK, false>(a, px, py, r, ri, sp[2 * j], sp[2 * j + 1], sg[j], j);
}

// Where one wave's sources come from: the scalar cache (ensemble_phi_kernel) or LDS (the traced chain).
struct ScalarSources {
    ConstF sp, sg;
    template <bool MASK>
    __device__ __forceinline__ void block(float (&a)[K], const float (&px)[K], const float (&py)[K], const float (&r)[K],
                                          const uint32_t (&ri)[K], uint32_t j0, uint32_t j1) const {
        block_sum<MASK>(a, px, py, r, ri, sp, sg, j0, j1);
    }
};
struct LdsSources {
    const float *sp, *sg;
    template <bool MASK>
    __device__ __forceinline__ void block(float (&a)[K], const float (&px)[K], const float (&py)[K], const float (&r)[K],
                                          const uint32_t (&ri)[K], uint32_t j0, uint32_t j1) const {
        block_sum_lds<MASK>(a, px, py, r, ri, sp, sg, j0, j1);
    }
};

// sum[k] = -Phi of the lane's K receivers (tile rows lane and lane + 64 of the tile that starts at receiver rb) over the
// n_src sources of their world, walked by ONE wave in the order potential_kernel's eight waves define: for w = 0..7 the
// blocks [w * per, (w + 1) * per) into a float64 s_w from 0.0, then 0.0 + s_0 + ... + s_7.  Only the sources that are
// the tile's own receivers run the masked body (a block is cut there).
template <typename SRC>
__device__ __forceinline__ void tile_potential(double (&sum)[K], const float (&px)[K], const float (&py)[K], const float (&r)[K],
                                               const uint32_t (&ri)[K], uint32_t rb, uint32_t n_src, const SRC &src) {
    float a[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        a[k] = 0.0f;
        sum[k] = 0.0;
    }
    const uint32_t nblocks = (n_src + BLOCK - 1) / BLOCK;
    const uint32_t per = (nblocks + W - 1) / W;
#pragma unroll 1
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t b_lo = min(w * per, nblocks);
        const uint32_t b_hi = min(b_lo + per, nblocks);
        double s[K];
#pragma unroll
        for (int k = 0; k < K; k++) s[k] = 0.0;
#pragma unroll 1
        for (uint32_t b = b_lo; b < b_hi; b++) {
            const uint32_t j0 = b * BLOCK, j1 = min(j0 + BLOCK, n_src);
            // [j0, m0) before, [m0, m1) the tile's own indices (masked), [m1, j1) after: the same pairs in the same order
            // as one block_sum over [j0, j1), and m0, m1 are multiples of 128 or an end of the block
            const uint32_t m0 = min(max(rb, j0), j1), m1 = min(max(rb + TILE, j0), j1);
#pragma unroll 1
            for (uint32_t seg = 0; seg < 3; seg++) {
                if (seg == 1)
                    src.template block<true>(a, px, py, r, ri, m0, m1);
                else
                    src.template block<false>(a, px, py, r, ri, seg ? m1 : j0, seg ? j1 : m0);
            }
#pragma unroll
            for (int k = 0; k < K; k++) {
                s[k] += (double)a[k];
                a[k] = 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < K; k++) sum[k] += s[k];
    }
}

// The eight float64 terms of receiver i of a tile, in diag_sums.h order.  A dead lane (past the last receiver) reads
// particle c = 0 and contributes exact zeros, every one of them by a select: particle 0 may hold anything (include/
// nbody_diag.h "Non-finite state"), and the 0 * inf or 0 * NaN of a dead lane must not reach the sum.  For finite data a
// product with m = 0 was a zero too, of either sign; the tile rows are added up from +0.0 (reduce_rows), where the sign
// of a zero term cannot show.
__device__ __forceinline__ void energy_terms(double (&e)[QTY], bool live, double phi, const float *mass, const float2 *pos,
                                             const float2 *vel, uint32_t i) {
    const uint32_t c = live ? i : 0u;
    const double m = (double)mass[c];
    const float2 x = pos[c], v = vel[c];
    const double vx = v.x, vy = v.y, xx = x.x, xy = x.y;
    e[0] = live ? m * phi : 0.0;
    e[1] = live ? m * (vx * vx + vy * vy) : 0.0;
    e[2] = live ? m : 0.0;
    e[3] = live ? m * vx : 0.0;
    e[4] = live ? m * vy : 0.0;
    e[5] = live ? m * (xx * vy - xy * vx) : 0.0;
    e[6] = live ? m * xx : 0.0;
    e[7] = live ? m * xy : 0.0;
}

// potential_kernel's tree over the 128 rows of a tile held by one wave: half = 64 is rows lane and lane + 64 (the lane's
// own two receivers), the other six levels cross lanes.  Lane 0 ends with the tile's row in t[].
__device__ __forceinline__ void tile_tree(double (&t)[QTY], const double (&e)[K][QTY]) {
#pragma unroll
    for (int q = 0; q < QTY; q++) t[q] = e[0][q] + e[1][q];
#pragma unroll
    for (int half = WAVE / 2; half > 0; half /= 2) {
#pragma unroll
        for (int q = 0; q < QTY; q++) t[q] = t[q] + __shfl_down(t[q], half, WAVE);   // exact for lanes < half
    }
}

// One workgroup of REDUCE_THREADS: out[q] = sum over the `rows` tile rows of quantity q.  Thread t of quantity q = t / 32
// adds rows [l * chunk, (l + 1) * chunk), l = t % 32, in index order; the 32 partial sums meet in a fixed tree.
__device__ __forceinline__ void reduce_rows(const double *slab, uint32_t rows, double *out) {
    constexpr uint32_t LANES = REDUCE_THREADS / QTY;
    __shared__ double red[QTY][LANES];
    const uint32_t q = threadIdx.x / LANES, l = threadIdx.x % LANES;
    const uint32_t chunk = (rows + LANES - 1) / LANES;
    const uint32_t lo = min(l * chunk, rows), hi = min(lo + chunk, rows);
    double s = 0.0;
    for (uint32_t row = lo; row < hi; row++) s += slab[(size_t)row * QTY + q];
    red[q][l] = s;
    __syncthreads();
    for (uint32_t half = LANES / 2; half > 0; half /= 2) {
        if (l < half) red[q][l] = red[q][l] + red[q][l + half];
        __syncthreads();
    }
    if (l == 0) out[q] = red[q][0];
}

// reduce_rows for threads t < REDUCE_THREADS of a LARGER workgroup (the traced chain: no workgroup barrier, no static LDS
// of its own): the 32 threads of a quantity are half a wave, so their tree runs through the cross-lane network.  The
// same partial sums meet in the same order -- level `half` adds lane l + half into lane l, exact for l < half, which is
// all the next level reads -- so out[] has reduce_rows' bits.  `slab` may be LDS.
__device__ __forceinline__ void reduce_rows_shfl(const double *slab, uint32_t rows, double *out, uint32_t t) {
    constexpr uint32_t LANES = REDUCE_THREADS / QTY;
    static_assert(LANES == 32 && WAVE % LANES == 0, "one quantity per half wave");
    const uint32_t q = t / LANES, l = t % LANES;
    const uint32_t chunk = (rows + LANES - 1) / LANES;
    const uint32_t lo = min(l * chunk, rows), hi = min(lo + chunk, rows);
    double s = 0.0;
    for (uint32_t row = lo; row < hi; row++) s += slab[(size_t)row * QTY + q];
    for (uint32_t half = LANES / 2; half > 0; half /= 2) s = s + __shfl_down(s, half, LANES);
    if (l == 0) out[q] = s;
}

}  // namespace nbd
