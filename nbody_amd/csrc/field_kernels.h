// field_kernels.h -- the device statements field.hip (one world), batch_field.hip (every member of an ensemble) and tidal.hip
// (the tidal tensor of both) share: the three quantity policies with their pair statements, the sampler's parameters, how a lane loads and stores its two samples,
// and the sum of one source slice.  The definitions and the summation order are stated at the head of
// field.hip; a result is defined by that order, so every kernel built from these statements gives the same bits.
// Device code: include it from a .hip file after diag_common.h.
#pragma once

#include "pipeline_internal.h"
#include "diag_common.h"
#include "field_common.h"
#include "interaction_asm.h"

namespace nb {
namespace field {

using namespace nbd;

constexpr int WAVES_MAX = 4;   // one wave per tile: tiles (waves) per workgroup

struct Params {
    const float2 *pos;     // pos[cur]: the latest state
    const float *src_gm;   // G * m_j, j < n_src
    uint32_t n_src;        // sources [0, M)
    const float *in;       // probes: (x, y) pairs; map: width column coordinates, then height row coordinates
    uint32_t n;            // samples
    uint32_t width;        // map only
    float soft;
    void *out;             // Q::Out of sample i, i < n
};

// Phi: diag_common.h's unmasked pair with the softening as every sample's radius
struct Potential {
    static constexpr int C = 1;     // running sums per sample
    static constexpr int OUT = 1;   // floats stored per sample
    typedef float Out;
    static constexpr const char *NOUN = "field";
    static constexpr int SimPipeline::*SHAPE = &SimPipeline::field_shape;

    // sources [j0, j1) of one block added to a[0][]
    static __device__ __forceinline__ void block(float (&a)[C][K], const float (&px)[K], const float (&py)[K], float s, ConstF sp,
                                                 ConstF sg, uint32_t j0, uint32_t j1) {
        float r[K];
        uint32_t ri[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            r[k] = s;
            ri[k] = 0;   // read by the masked body only
        }
        block_sum<false>(a[0], px, py, r, ri, sp, sg, j0, j1);
    }
    static __device__ __forceinline__ Out result(const double (&sum)[C]) { return (float)-sum[0]; }
    static __device__ __forceinline__ Out nan() { return __builtin_nanf(""); }
};

// g: the step kernels' own statement (interaction_asm.h NB_INTERACTION2_ASM: the lane's two samples against one wave-uniform
// source, both v_rsq_f32 inside one raised-priority window) with r0 = r1 = s
struct Acceleration {
    static constexpr int C = 2;
    static constexpr int OUT = 2;
    typedef float2 Out;
    static constexpr const char *NOUN = "gravity";
    static constexpr int SimPipeline::*SHAPE = &SimPipeline::gravity_shape;

    static __device__ __forceinline__ void pair2(float (&a)[C][K], const float (&px)[K], const float (&py)[K], float s, float sx, float sy,
                                                 float g) {
        asm(NB_INTERACTION2_ASM
            : [ax0] "+v"(a[0][0]), [ay0] "+v"(a[1][0]), [ax1] "+v"(a[0][1]), [ay1] "+v"(a[1][1])
            : [sx] "s"(sx), [sy] "s"(sy), [g] "s"(g), [px0] "v"(px[0]), [py0] "v"(py[0]), [r0] "v"(s), [px1] "v"(px[1]), [py1] "v"(py[1]),
              [r1] "v"(s)
            : NB_CLOBBERS2);
    }
    // sources [j0, j1) of one block added to a[0][] (x) and a[1][] (y): the walk of diag_common.h's block_sum, one register set
    static __device__ __forceinline__ void block(float (&a)[C][K], const float (&px)[K], const float (&py)[K], float s, ConstF sp,
                                                 ConstF sg, uint32_t j0, uint32_t j1) {
        uint32_t j = j0;
        for (; j + 8 <= j1; j += 8) {
            const v16f P = cload<v16f>(sp + 2 * (size_t)j);
            const v8f G = cload<v8f>(sg + j);
#pragma unroll
            for (int u = 0; u < 8; u++) pair2(a, px, py, s, P[2 * u], P[2 * u + 1], G[u]);
        }
        for (; j < j1; j++) pair2(a, px, py, s, sp[2 * (size_t)j], sp[2 * (size_t)j + 1], sg[j]);
    }
    static __device__ __forceinline__ Out result(const double (&sum)[C]) { return make_float2((float)sum[0], (float)sum[1]); }
    static __device__ __forceinline__ Out nan() { return make_float2(__builtin_nanf(""), __builtin_nanf("")); }
};
static_assert(K == 2, "NB_INTERACTION2_ASM is the statement for two samples per lane");

// T = dg/dp (include/nbody_tidal.h): four running sums per sample, three floats stored.  With w = G*m u^3 (the force
// statement's factor, same roundings) and w5 = w * u^2 the sums are A = sum dx (dx w5), B = sum dx (dy w5), C = sum dy (dy w5)
// and D = sum w; the factor 3 and the difference 3A - D of a diagonal component are formed in float64 from the float64 totals
// (result()), so the fp32 sums A, C and D hold terms of one sign and the error scales with the parts, not with what is left
// of them.  One statement for the lane's two samples against one wave-uniform source, both v_rsq_f32 inside one
// raised-priority window like NB_INTERACTION2_ASM; every product rounded, v_fma / v_fmac only where written:
//     dx = sx - px;  dy = sy - py;  q = fma(dy, dy, fma(dx, dx, s));  u = rsq(q);  u2 = u * u
//     w  = (g * u) * u2;  D += w;  w5 = w * u2;  tx = dx * w5;  ty = dy * w5
//     A  = fma(dx, tx, A);  B = fma(dx, ty, B);  C = fma(dy, ty, C)
// 14 VALU instructions and one v_rsq_f32 per pair.
#define NB_TIDAL_TAIL_ASM(dx, dy, u, A, B, C, D)     \
    "v_mul_f32 %[w], %[g], " u "\n\t"               \
    "v_mul_f32 %[u2], " u ", " u "\n\t"             \
    "v_mul_f32 %[w], %[w], %[u2]\n\t"               \
    "v_add_f32 " D ", " D ", %[w]\n\t"              \
    "v_mul_f32 %[w], %[w], %[u2]\n\t"               \
    "v_mul_f32 %[u2], " dx ", %[w]\n\t"             \
    "v_mul_f32 %[w], " dy ", %[w]\n\t"              \
    "v_fmac_f32 " A ", " dx ", %[u2]\n\t"           \
    "v_fmac_f32 " B ", " dx ", %[w]\n\t"            \
    "v_fmac_f32 " C ", " dy ", %[w]"
#define NB_TIDAL2_ASM                                \
    "v_sub_f32 %[dx0], %[sx], %[px0]\n\t"           \
    "v_sub_f32 %[dy0], %[sy], %[py0]\n\t"           \
    "v_fma_f32 %[q0], %[dx0], %[dx0], %[s]\n\t"     \
    "v_fmac_f32 %[q0], %[dy0], %[dy0]\n\t"          \
    "v_sub_f32 %[dx1], %[sx], %[px1]\n\t"           \
    "v_sub_f32 %[dy1], %[sy], %[py1]\n\t"           \
    "v_fma_f32 %[q1], %[dx1], %[dx1], %[s]\n\t"     \
    "v_fmac_f32 %[q1], %[dy1], %[dy1]\n\t"          \
    "s_setprio 3\n\t"                               \
    "v_rsq_f32 %[q0], %[q0]\n\t"                    \
    "v_rsq_f32 %[q1], %[q1]\n\t"                    \
    "s_setprio 0\n\t"                               \
    NB_TIDAL_TAIL_ASM("%[dx0]", "%[dy0]", "%[q0]", "%[a0]", "%[b0]", "%[c0]", "%[d0]") "\n\t" \
    NB_TIDAL_TAIL_ASM("%[dx1]", "%[dy1]", "%[q1]", "%[a1]", "%[b1]", "%[c1]", "%[d1]")

struct Tidal {
    static constexpr int C = 4;     // A, B, C, D above
    static constexpr int OUT = 3;   // xx, xy, yy
    struct Out {
        float xx, xy, yy;
    };
    static constexpr const char *NOUN = "tidal";
    static constexpr int SimPipeline::*SHAPE = &SimPipeline::tidal_shape;

    static __device__ __forceinline__ void pair2(float (&a)[C][K], const float (&px)[K], const float (&py)[K], float s, float sx, float sy,
                                                 float g) {
        float dx0, dy0, q0, dx1, dy1, q1, w, u2;
        asm(NB_TIDAL2_ASM
            : [a0] "+v"(a[0][0]), [b0] "+v"(a[1][0]), [c0] "+v"(a[2][0]), [d0] "+v"(a[3][0]), [a1] "+v"(a[0][1]), [b1] "+v"(a[1][1]),
              [c1] "+v"(a[2][1]), [d1] "+v"(a[3][1]), [dx0] "=&v"(dx0), [dy0] "=&v"(dy0), [q0] "=&v"(q0), [dx1] "=&v"(dx1),
              [dy1] "=&v"(dy1), [q1] "=&v"(q1), [w] "=&v"(w), [u2] "=&v"(u2)
            : [sx] "s"(sx), [sy] "s"(sy), [g] "s"(g), [px0] "v"(px[0]), [py0] "v"(py[0]), [px1] "v"(px[1]), [py1] "v"(py[1]), [s] "v"(s));
    }
    // sources [j0, j1) of one block: the walk of Acceleration::block
    static __device__ __forceinline__ void block(float (&a)[C][K], const float (&px)[K], const float (&py)[K], float s, ConstF sp,
                                                 ConstF sg, uint32_t j0, uint32_t j1) {
        uint32_t j = j0;
        for (; j + 8 <= j1; j += 8) {
            const v16f P = cload<v16f>(sp + 2 * (size_t)j);
            const v8f G = cload<v8f>(sg + j);
#pragma unroll
            for (int u = 0; u < 8; u++) pair2(a, px, py, s, P[2 * u], P[2 * u + 1], G[u]);
        }
        for (; j < j1; j++) pair2(a, px, py, s, sp[2 * (size_t)j], sp[2 * (size_t)j + 1], sg[j]);
    }
    // float64: the factor 3 and the cancellation of a diagonal component; each component rounded once
    static __device__ __forceinline__ Out result(const double (&sum)[C]) {
        return Out{(float)(3.0 * sum[0] - sum[3]), (float)(3.0 * sum[1]), (float)(3.0 * sum[2] - sum[3])};
    }
    static __device__ __forceinline__ Out nan() { return Out{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")}; }
};
static_assert(sizeof(Tidal::Out) == Tidal::OUT * sizeof(float), "three packed floats per sample");

// the K samples of this lane: tile rows lane and lane + 64; tail lanes redo the last sample, their results are dropped
template <bool MAP>
__device__ __forceinline__ void load_samples(const Params &p, uint32_t rb, uint32_t lane, float (&px)[K], float (&py)[K]) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        uint32_t i = rb + k * WAVE + lane;
        i = i < p.n ? i : p.n - 1;
        if constexpr (MAP) {
            const uint32_t row = i / p.width, col = i - row * p.width;
            px[k] = p.in[col];
            py[k] = p.in[p.width + row];
        } else {
            const float2 q = reinterpret_cast<const float2 *>(p.in)[i];
            px[k] = q.x;
            py[k] = q.y;
        }
    }
}

template <typename Q>
__device__ __forceinline__ void store_sample(const Params &p, uint32_t i, float x, float y, const double (&sum)[Q::C]) {
    if (i >= p.n) return;
    const bool finite = nb_render_finite(x) && nb_render_finite(y);
    const typename Q::Out v = Q::result(sum);
    static_cast<typename Q::Out *>(p.out)[i] = finite ? v : Q::nan();
}

// slice w of the W source slices, in whole blocks: [b_lo, b_hi) added to the float64 sums s[][] (from whatever they hold),
// one fp32 block sum at a time
template <typename Q>
__device__ __forceinline__ void slice_sum(double (&s)[Q::C][K], const float (&px)[K], const float (&py)[K], const Params &p, uint32_t w) {
    const uint32_t nblocks = (p.n_src + BLOCK - 1) / BLOCK;
    const uint32_t per = (nblocks + W - 1) / W;
    const uint32_t b_lo = min(w * per, nblocks);
    const uint32_t b_hi = min(b_lo + per, nblocks);
    const ConstF sp = (ConstF)(uintptr_t)p.pos, sg = (ConstF)(uintptr_t)p.src_gm;
    float a[Q::C][K];
#pragma unroll
    for (int k = 0; k < K; k++)
        for (int c = 0; c < Q::C; c++) a[c][k] = 0.0f;
#pragma unroll 1
    for (uint32_t b = b_lo; b < b_hi; b++) {
        const uint32_t j0 = b * BLOCK, j1 = min(j0 + BLOCK, p.n_src);
        Q::block(a, px, py, p.soft, sp, sg, j0, j1);
#pragma unroll
        for (int k = 0; k < K; k++)
            for (int c = 0; c < Q::C; c++) {
                s[c][k] += (double)a[c][k];
                a[c][k] = 0.0f;
            }
    }
}

}  // namespace field
}  // namespace nb
