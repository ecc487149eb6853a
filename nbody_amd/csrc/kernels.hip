// kernels.hip -- gfx950 (CDNA4, wave64) kernels of the direct N-body step.
//
// Replaces the reference's GLSL compute shader (reference src/shader/particle_cs.glsl:28-55), which
// walks all sources per thread straight from global memory as 32-byte AoS records.  Here:
//
//   * one LANE owns K receivers (register blocking), one WAVE owns 64*K receivers and a 1/W slice of the
//     sources, one WORKGROUP = W waves over the same 64*K receivers; the W partial sums meet in LDS in a
//     fixed order (deterministic results), then the workgroup integrates and stores; a launch may also cut the
//     sources into `split` parts (gridDim.y) whose sums a small finish kernel adds, and slices are whole granules
//     of 64 sources or, for latency-bound launches on the scalar-cache route, of 32 / 16 / 8 (StepParams::unit);
//   * sources reach the VALU wave-uniformly, 12 bytes each (x, y, G*m), by one of two routes:
//       VARIANT_LDS   each wave stages 64-source tiles in its own LDS slab: coalesced float2/float loads
//                     (one source per lane), ds_write_b64 + b32, then broadcast ds_read_b128 (six per 8
//                     sources); double-buffered, no workgroup barrier in the loop;
//       VARIANT_SMEM  the wave reads its slice through the scalar cache (s_load_dwordx8/x16) so sources
//                     arrive in SGPRs and feed the VALU as scalar operands; no LDS, no VGPR staging;
//   * per interaction: 2 sub (dx, dy), 2 fma (dist^2 + receiver radius), v_rsq_f32, 3 mul, 2 fma into the
//     accumulators = 10 plain VALU instructions, none packed, against the reference's 14 counted flops
//     (SURVEY.md 8d keeps 14 as the roofline convention);
//   * sums are two-level (plain over blocks of 256 sources, then Kahan over the block totals), so the fp32 result
//     stays within ~4e-7 * sum|contribution| (rms) of the float64 sum at any N and launch shape, 180x closer than
//     the reference's own AVX sums at N = 2^20;
//   * the integrator keeps the reference's rounding (mul, then add; sim_cpu.c:191-193 /
//     particle_cs.glsl:51-52), the force loop does not (rsq + fma instead of sqrt, div, mul, add):
//     DESIGN.md states the tolerance.
//
// fp32 throughout.  No MFMA: the loop is rsqrt/fma on independent (receiver, source) pairs, not a contraction.
//
// This file holds the force path and nothing else: it, step_tile.inc, kernels.h and interaction_asm.h are the sources whose hash ties a
// PMC profile to the code that was profiled (benchlib.KERNEL_SOURCES), so every device function a force kernel compiles
// lives in one of the three -- but for the record phase of the traced ensemble chain, which is the diagnostics' arithmetic
// and comes from diag_common.h.  Which shape a launch gets is host arithmetic in launch_shape.hip; the AoS <-> SoA
// converters, pads and fills are convert.hip.
#include "kernels.h"
#include "diag_common.h"
#include "interaction_asm.h"
#include "launch_shape.h"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace nb {
namespace {

constexpr int WAVE = 64;
constexpr int CHUNK = 64;  // sources per staged tile = one per lane
constexpr int CLOSE_EVERY = 4;  // tiles per summation block: plain sums over 256 sources, Kahan across blocks

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v8f __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

typedef float f2v __attribute__((ext_vector_type(2)));

template <int K>
struct Receivers {
    f2v p[K];    // position (x, y): one aligned VGPR pair, the operand of v_pk_add_f32
    float r[K];  // radius (softening term)
    f2v a[K];    // running sums (ax, ay) of the current block of 256 sources: operand of v_pk_fma_f32
    f2v s[K];    // sums of the finished blocks ...
    f2v c[K];    // ... and their Kahan compensation
    // Two-level summation: 256 terms per block in a[], then the block totals are added to s[] with
    // compensated (Kahan) summation, 8 adds per block per receiver (0.4 % of a block's 2048 instructions).
    // A plain running sum of 10^5..10^6 same-signed pulls loses 4-5 digits (the reference's 8-lane AVX sums do:
    // profiles/r01_accuracy_vs_f64_and_avx.txt); even a plain sum of chunk totals drifts with the slice length
    // (profiles/r01_accuracy2_shapes_before_kahan.txt).  This way the error no longer depends on N or on the
    // launch shape.  Built without fast-math and with -ffp-contract=off, so the compensation survives.
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < K; k++) a[k] = s[k] = c[k] = f2v{0.0f, 0.0f};
    }
    __device__ __forceinline__ void close_chunk() {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const f2v y = a[k] - c[k];
            const f2v t = s[k] + y;
            const f2v cn = (t - s[k]) - y;
            // a block that added exactly nothing (zero-mass pad sources of a sharded launch) must leave the
            // state untouched, or padded and unpadded launches would differ in the last bit
            const bool lx = a[k].x != 0.0f, ly = a[k].y != 0.0f;
            // a total that has left the finite range carries no compensation ((inf - s) - inf is NaN, and the next block
            // would turn a sum of +-inf into NaN, which the reference's plain sums do not: include/nbody_hip.h "Non-finite
            // state").  A select on t: +-inf then survives finite blocks, +inf meets -inf as NaN, NaN stays NaN.
            const bool fx = __builtin_fabsf(t.x) < __builtin_inff(), fy = __builtin_fabsf(t.y) < __builtin_inff();
            c[k].x = lx ? (fx ? cn.x : 0.0f) : c[k].x;
            c[k].y = ly ? (fy ? cn.y : 0.0f) : c[k].y;
            s[k].x = lx ? t.x : s[k].x;
            s[k].y = ly ? t.y : s[k].y;
            a[k] = f2v{0.0f, 0.0f};
        }
    }
};

// One source against the K receivers of this lane.  sxy/sg are wave-uniform (SGPRs).
//
// The ten VALU instructions of an interaction are written out as one asm statement per (source, receiver):
//     v_sub_f32   dx  = sx - x
//     v_sub_f32   dy  = sy - y
//     v_fma_f32   q   = dx * dx + radius           softening: + radius of the RECEIVER, not squared
//     v_fmac_f32  q  += dy * dy
//     v_rsq_f32   q   = 1 / sqrt(q)                1 ulp; issued at raised wave priority
//     v_mul_f32   u   = (G*m) * q                  G*m straight from its SGPR
//     v_mul_f32   t   = q * q
//     v_mul_f32   u   = u * t                      G*m / dist^3
//     v_fmac_f32  ax += dx * u
//     v_fmac_f32  ay += dy * u
// = 9 plain instructions (2 issue cycles each) + one quarter-rate transcendental (8) = 26 cycles per wave-interaction,
// the floor of this mix; the kernel runs at 27.2 (profiles/r02_ab_plain_body.txt).
// No packed instruction: round 1 shipped v_pk_add_f32 for (dx, dy) and v_pk_fma_f32 for the accumulation -- two fewer
// instructions, the same nominal cycles -- and measured 28.4-28.9 cycles; the all-plain body is 4.5 % faster on every
// box tried (51.2 -> 48.8 ms per launch at N = 2^20), while unpacking only one of the two is slower than either
// (+1 % and +12 %): packed f32 costs more than its two halves when it sits between plain and transcendental
// instructions (MI355X_MICROARCH.md notes the same beside MFMAs).
// Why asm: (1) left to hipcc, the multiplies become two v_pk_mul_f32 plus a v_mov, and both the schedule and
// the register count of the unrolled loop swing with unrelated edits (55..75 VGPRs; 65 halves the occupancy of a
// 1024-thread workgroup): the same loop measured anywhere from 105 to 151 ms per step at N = 2^20
// (profiles/r01_sweep_auto_split.txt, r01_sweep8_full_asm_nops_alignment.txt).  One fixed sequence on five fixed
// temporaries cannot drift.  (2) A v_rsq_f32 that lands between other waves' plain VALU
// instructions costs ~16 cycles instead of 8 on gfx950; raising the wave priority for just that instruction buys
// 6 % with the packed body and 13 % with this one (profiles/r01_ubench5_setprio_rsq.txt,
// r01_sweep9_nops_and_static_priority.txt, r02_ab_plain_body.txt; static per-wave priorities instead are 3x SLOWER;
// priority 1 instead of 3, or the window opened one instruction earlier: within 0.3 %).  (3) gfx950 needs one wait
// state between a transcendental and the VALU instruction that reads its result, and hipcc cannot pad inside asm:
// the s_setprio 0 that follows the rsq IS that wait state (an earlier version with nothing in between read stale
// values; the parity tests caught it, and tests/test_isa.py now checks the ISA).  The other dependent pairs are
// ordinary VALU read-after-write, which the hardware interlocks.  (4) One statement per interaction: hipcc pads each
// asm boundary with an s_nop (56 + 4 bytes).  Each interaction is a serial dependency chain on purpose: with 8 waves per
// SIMD the other waves fill the gaps, and interleaved or software-pipelined orders measured slower
// (profiles/r01_ubench3_hand_scheduled_bodies.txt).
// The statement is pure (no memory, not volatile); 12 instructions, 56 bytes, all in their short encodings.
// Temporaries (clobbered): dx = v30, dy = v31, t = v32, q = v33, u = v36 (v37 stays on the list: generated tuning
// bodies use it).
// (the statement text itself: interaction_asm.h, shared with the clock probe)

// SRC_IN_SGPR: the source sits in SGPRs (scalar-cache route) or in VGPRs holding a wave-uniform value
// (LDS broadcast reads); the instructions are the same, only the operand class differs.
// One statement per K; SRC is the constraint letter of the three source operands.
#define NB_INTERACT2(SRC)                                                                                                       \
    asm(NB_INTERACTION2_ASM                                                                                                     \
        : [ax0] "+v"(R.a[0].x), [ay0] "+v"(R.a[0].y), [ax1] "+v"(R.a[1].x), [ay1] "+v"(R.a[1].y)                                \
        : [sx] SRC(sxy.x), [sy] SRC(sxy.y), [g] SRC(sg), [px0] "v"(R.p[0].x), [py0] "v"(R.p[0].y), [r0] "v"(R.r[0]),            \
          [px1] "v"(R.p[1].x), [py1] "v"(R.p[1].y), [r1] "v"(R.r[1])                                                            \
        : NB_CLOBBERS2)
#define NB_INTERACT1(SRC)                                                                                                       \
    asm(NB_INTERACTION_ASM                                                                                                      \
        : [ax] "+v"(R.a[k].x), [ay] "+v"(R.a[k].y)                                                                              \
        : [sx] SRC(sxy.x), [sy] SRC(sxy.y), [g] SRC(sg), [px] "v"(R.p[k].x), [py] "v"(R.p[k].y), [r] "v"(R.r[k])                \
        : NB_CLOBBERS)
template <int K, bool SRC_IN_SGPR>
__device__ __forceinline__ void interact(Receivers<K> &R, f2v sxy, float sg) {
    if constexpr (K == 2) {
        if constexpr (SRC_IN_SGPR) NB_INTERACT2("s");
        else NB_INTERACT2("v");
        return;
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        if constexpr (SRC_IN_SGPR) NB_INTERACT1("s");
        else NB_INTERACT1("v");
    }
}
#undef NB_INTERACT2
#undef NB_INTERACT1

// 8 sources (x,y interleaved in P, G*m in G) against the K receivers: 8*K interaction statements, source-major.
// (Schedule experiments replace this one function from outside the product tree: tools/exp_body_hook.h, force-included
// by tools/build_variants.sh, defines NB_INTERACT8_OVERRIDE and supplies its own.)
#ifndef NB_INTERACT8_OVERRIDE
template <int K, bool SRC_IN_SGPR, typename VP, typename VG>
__device__ __forceinline__ void interact8(Receivers<K> &R, const VP &P, const VG &G) {
#pragma unroll
    for (int u = 0; u < 8; u++) interact<K, SRC_IN_SGPR>(R, f2v{P[2 * u], P[2 * u + 1]}, G[u]);
}
#else
NB_INTERACT8_OVERRIDE
#endif

// A wave-uniform load from the source arrays becomes a scalar load (s_load_dwordx8/x16) only while the compiler can prove
// that nothing in the kernel has written memory before it: true by construction, since every store of the step kernel
// sits in its epilogue, after the last source load.
// The dealt kernel draws its ticket (an atomic, an LDS word, a barrier) BEFORE the loop, so the proof is gone there;
// CONSTANT = true states the fact instead: the load goes through the constant address space, which promises that nothing
// writes the location while the kernel runs -- true of the source arrays, the snapshot of the previous step, in every
// launch -- and a wave-uniform load from it is always a scalar load.
template <typename V, bool CONSTANT = false>
__device__ __forceinline__ V src_load(const float *ptr) {
    if constexpr (CONSTANT) return *(const __attribute__((address_space(4))) V *)(ptr);
    else return *reinterpret_cast<const V *>(ptr);
}

// Slot of logical receiver i (see StepParams::recv_split).
__device__ __forceinline__ uint32_t receiver_slot(const StepParams &p, uint32_t i) {
    return i + (i >= p.recv_split ? p.recv_gap : 0u);
}

// Map a position v of the concatenated source ranges to an index of src_pos/src_gm.
__device__ __forceinline__ uint32_t source_index(const StepParams &p, uint32_t v, uint32_t n0) {
    return v < n0 ? p.src_begin[0] + v : p.src_begin[1] + (v - n0);
}

// ---- one copy of each rule the launch paths must agree on bit for bit --------------------------------------------------
// The helpers take values their callers have already loaded: where and when each load is issued is a measured choice of
// the call site (finish_kernel's all-at-once part loads, lane_split_kernel's early velocity fetch).

__device__ __forceinline__ float2 add_rn(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }

// semi-implicit Euler with the reference's roundings (mul, then add; sim_cpu.c:191-193 / particle_cs.glsl:51-52):
// vel += acc*dt; pos += vel*dt
__device__ __forceinline__ void integrate(float2 a, float dt, float2 &v, float2 &q) {
    v.x = __fadd_rn(v.x, __fmul_rn(a.x, dt));
    v.y = __fadd_rn(v.y, __fmul_rn(a.y, dt));
    q.x = __fadd_rn(q.x, __fmul_rn(v.x, dt));
    q.y = __fadd_rn(q.y, __fmul_rn(v.y, dt));
}

// the new velocity and position of receiver slot i (and the position's copy in the next gathered source array)
__device__ __forceinline__ void store_moved(const StepParams &p, uint32_t i, float2 v, float2 q) {
    p.vel[i] = v;
    p.pos_out[i] = q;
    if (i < p.n_mirror) p.mirror[i] = q;
}

// Receiver slot i with its sum `a` and its old acc / vel / pos (a0, v, q) in registers: carry in, store acc, integrate.
__device__ __forceinline__ void finish_loaded(const StepParams &p, uint32_t i, float2 a, float2 a0, float2 v, float2 q, float dt) {
    if (p.flags & STEP_ACC_IN) a = add_rn(a0, a);
    p.acc[i] = a;
    if (p.flags & STEP_NO_FINALIZE) return;
    integrate(a, dt, v, q);
    store_moved(p, i, v, q);
}

// One term of the part-order sum of a split step, 0 + p0 + p1 + ... with the roundings of a sequential loop.  Callers load
// all MAX_SPLIT parts before the first add (unused slots re-read the last part) and pass live = s < split: the unused
// ones are dropped by a select, not a branch.  Per term, with the sum in two floats: a helper that took the whole array
// and returned a float2 let the compiler wait for the first part before issuing the loads of the others.
__device__ __forceinline__ void add_part(float &sx, float &sy, float2 part, bool live) {
    const float nx = __fadd_rn(sx, part.x), ny = __fadd_rn(sy, part.y);
    sx = live ? nx : sx;
    sy = live ? ny : sy;
}

// The partial sums of n source slices of one receiver, in slice (= wave) order: first[0], first[stride], ...
__device__ __forceinline__ float2 wave_sum(const float2 *first, uint32_t stride, uint32_t n) {
    float sx = 0.0f, sy = 0.0f;
    for (uint32_t s = 0; s < n; s++) {
        const float2 t = first[s * stride];
        sx = __fadd_rn(sx, t.x);
        sy = __fadd_rn(sy, t.y);
    }
    return make_float2(sx, sy);
}

// The source slice [lo, hi) of one wave (or lane group): the `total` sources, in whole granules of `unit` sources, are cut
// into `parts` parts (the source split of a step; 1 elsewhere), and part `part` into n slices, of which this is slice i.
// The last granule may be ragged and trailing slices are empty (hi == lo, also past a ragged last granule: 7 granules
// of 8 over 16 slices, 50 sources, start slice 7 at 56).  Every launch path slices with this, which is what makes their
// summation orders agree.
struct SourceSlice {
    uint32_t lo, hi;
};
__device__ __forceinline__ SourceSlice source_slice(uint32_t total, uint32_t unit, uint32_t parts, uint32_t part, uint32_t n,
                                                    uint32_t i) {
    const uint32_t nunits = (total + unit - 1) / unit;
    const uint32_t per_part = (nunits + parts - 1) / parts;
    const uint32_t part_lo = min(part * per_part, nunits);
    const uint32_t part_hi = min(part_lo + per_part, nunits);
    const uint32_t per = (part_hi - part_lo + n - 1) / n;
    const uint32_t u_lo = min(part_lo + i * per, part_hi);
    const uint32_t u_hi = min(u_lo + per, part_hi);
    const uint32_t lo = u_lo * unit;
    return {lo, max(min(u_hi * unit, total), lo)};
}

// Epilogue of one receiver of an unsplit launch: acc is loaded only to carry it in, vel / pos only to integrate.
__device__ __forceinline__ void finish_receiver(const StepParams &p, uint32_t logical, float sx, float sy, float dt) {
    if (logical >= p.n_recv) return;
    const uint32_t i = receiver_slot(p, logical);
    float2 a = make_float2(sx, sy);
    if (p.flags & STEP_ACC_IN) a = add_rn(p.acc[i], a);
    p.acc[i] = a;
    if (p.flags & STEP_NO_FINALIZE) return;
    float2 v = p.vel[i], q = p.pos_in[i];
    integrate(a, dt, v, q);
    store_moved(p, i, v, q);
}

// Second kernel of a split step: one thread per receiver adds the parts in part order and finishes.
// The kernel is pure latency -- a handful of loads, a handful of adds, three stores -- and what it reads was just
// written by other CUs (the parts) or other XCDs (acc, vel, pos), so every load is a 500-900 cycle trip to the
// Infinity Cache or HBM.  Issued one after the other behind a loop with a run-time trip count they cost `split` + 2 such
// trips in a row (measured: 4.0 us per launch at N = 10 000 / 5 parts, 5.0 us at 50 000 / 7 parts, of a 21 us step:
// profiles/r02_mid_n_pmc.txt); issued all at once, before the first use, they cost one.  Unused slots re-read the last
// part (always a valid address) and are dropped by a select, so the loads need no branch.
__global__ __launch_bounds__(256) void finish_kernel(const StepParams p) {
    const uint32_t logical = blockIdx.x * blockDim.x + threadIdx.x;
    if (logical >= p.n_recv) return;
    const uint32_t i = receiver_slot(p, logical);
    float2 part[MAX_SPLIT];
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)MAX_SPLIT; s++)
        part[s] = p.parts[(size_t)(s < p.split ? s : p.split - 1) * p.n_recv + logical];
    // clamped-to-valid addresses again: acc / vel / pos_in exist for every slot whatever the flags say
    const float2 a0 = p.acc[i];
    const float2 v0 = p.vel[i];
    const float2 q0 = p.pos_in[i];
    const float dt = *p.dt;
    float sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)MAX_SPLIT; s++) add_part(sx, sy, part[s], s < p.split);
    finish_loaded(p, i, make_float2(sx, sy), a0, v0, q0, dt);
}

// Everything must stay within 64 VGPRs: a 1024-thread workgroup puts 4 waves on every SIMD, so 65 VGPRs (7 waves
// per SIMD) would mean ONE resident workgroup per CU instead of two.  The asm body needs 36 (SMEM, K <= 2) / 62 (LDS);
// the second launch-bound argument (waves per SIMD) makes the limit explicit.  K = 4 then keeps its Kahan state in
// scratch, touched only at block closes outside the inner loop, and runs as fast as K = 2.
//
// A workgroup computes receiver tile blockIdx.x against source part blockIdx.y; the body is step_tile.inc.
template <int K, int W, int VARIANT, bool FUSED = false>
__global__ __launch_bounds__(WAVE *W, 8) void step_kernel(const StepParams p) {
    constexpr bool SRC_CONSTANT = false;   // nothing is stored before the loop: the source loads are scalar by themselves
    const uint32_t tile_x = blockIdx.x, part_y = blockIdx.y;
#include "step_tile.inc"
}

// The dealt launch ("deal" knob; step_chain.hip deal_applies): exactly the work of step_kernel<K, W, VARIANT_SMEM, false>,
// but a workgroup's (receiver tile, source part) is the next ticket of one counter, not its block index.  The hardware
// deals the workgroups of a grid to the eight XCDs in equal shares by block index, each XCD works through its own share
// at its own pace (profiles/r23_xcd_finish_probe.txt), and the odd XCDs hold 1-2 % less clock: the grid is therefore a
// little larger than the item count (p.deal_items + extra workgroups), a fast XCD reaches its last workgroups while
// tickets remain and takes real items, and the last workgroups of a slow XCD draw past the end and leave at once.  No
// loop, no workgroup waits for another, no data changes hands inside the launch: the parts meet in finish_kernel's own
// launch as before, and which workgroup computed an item cannot show in the result.  The draw that is the launch's last
// (gridDim.x - 1, empties included) puts the counter back to zero for the next launch, which sits behind a kernel
// boundary.  One LDS word and one barrier hand the ticket to every wave as a scalar.
template <int K, int W>
__global__ __launch_bounds__(WAVE *W, 8) void dealt_kernel(const StepParams p) {
    constexpr int VARIANT = VARIANT_SMEM;
    constexpr bool FUSED = false;
    constexpr bool SRC_CONSTANT = true;   // src_load: the ticket's atomic and LDS word come before the source loads
    __shared__ uint32_t drawn;
    if (threadIdx.x == 0) {
        const uint32_t t = __hip_atomic_fetch_add(p.deal, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == gridDim.x - 1) __hip_atomic_store(p.deal, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next launch
        drawn = t;
    }
    __syncthreads();
    const uint32_t ticket = __builtin_amdgcn_readfirstlane(drawn);
    const DealItem item = deal_item(ticket, p.deal_items / p.split, p.split);
    if (!item.live) return;   // the whole workgroup: the ticket is uniform
    const uint32_t tile_x = item.tile, part_y = item.part;
#include "step_tile.inc"
}

// ---- lane-split step: several source slices per receiver inside one wave -------------------------------------------
//
// Between the one-workgroup chain (N <= 256) and launches that fill the chip (N >~ 20 000) a step is bound by latency:
// the kernel boundary plus one wave's dependency chain over its slice of the sources.  The source split shortens the
// chain by giving a receiver tile to several workgroups -- and pays a second dependent kernel (the finish kernel,
// 1.7 us of boundary + ~1 us of its own) to add their sums.  Here the extra slices live INSIDE the wave instead: the 64
// lanes are `H` groups over the same 64 / H receivers, every group walks its own slice, and the W x H partial sums meet
// in LDS like the W of the ordinary kernel.  Lanes of different groups need different sources at the same time, so the
// source cannot be a wave-uniform scalar operand: the workgroup stages the sources in LDS, tile by tile (2 x 64 x W
// sources per tile, coalesced loads, fetched into registers one tile ahead), and every lane reads its own slice of the
// tile -- per-lane data is what LDS is for (cf. "Why the LDS-tile route trails").  K = 1, split = 1, slices in 8-source
// granules, Kahan block closes every 128 sources a lane has added.
//
// The body is a device function of the parameter block: lane_split_kernel runs it for one world, batch_lane_split_kernel
// (below) for member blockIdx.y of an ensemble.  blockIdx.x is the receiver tile in both.
template <int W, int H>
__device__ __forceinline__ void lane_split_body(const StepParams &p) {
    constexpr uint32_t R = WAVE / H;        // receivers per workgroup
    constexpr uint32_t V = W * H;           // source slices per receiver
    constexpr uint32_t T = 2 * WAVE * W;    // sources per staged tile: two per thread (12 KB at W = 8, 24 KB at W = 16)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float2 *sxy = reinterpret_cast<float2 *>(lds_raw);
    float *sgm = reinterpret_cast<float *>(sxy + T);
    float2 *partial = reinterpret_cast<float2 *>(sgm + T);   // [V][R], then [S][R]
    const uint32_t n0 = p.src_end[0] - p.src_begin[0];
    const uint32_t ntiles = (n0 + T - 1) / T;

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1);
    const uint32_t wid = tid >> 6;
    const uint32_t r = lane % R, h = lane / R;
    const uint32_t v = wid * H + h;         // this lane's slice of every tile
    const float dt = *p.dt;

    // tile t of the sources, two per thread, fetched into registers one tile ahead (coalesced float2 / float loads);
    // indices past the end are clamped -- the walk below never reads those LDS entries
    float2 q0 = make_float2(0.f, 0.f), q1 = q0;
    float m0 = 0.f, m1 = 0.f;
    auto fetch = [&](uint32_t t) {
        const uint32_t last = p.src_begin[0] + n0 - 1;
        const uint32_t j0 = min(p.src_begin[0] + t * T + tid, last), j1 = min(j0 + WAVE * W, last);
        q0 = p.src_pos[j0];
        q1 = p.src_pos[j1];
        m0 = p.src_gm[j0];
        m1 = p.src_gm[j1];
    };
    if (ntiles > 0) fetch(0);

    Receivers<1> Rv;
    {
        uint32_t i = blockIdx.x * R + r;
        i = i < p.n_recv ? i : p.n_recv - 1;  // tail lanes redo the last receiver; the epilogue masks them
        i = receiver_slot(p, i);
        const float2 q = p.pos_in[i];
        Rv.p[0] = f2v{q.x, q.y};
        Rv.r[0] = p.radius[i];
    }
    Rv.clear();
    // The integrating threads (first wave, lanes < R: lane == r there, so Rv.p IS their receiver's position) fetch the
    // velocity now: behind the reduction it would be one more memory round trip (~0.3 us of a ~3 us step) on the
    // critical path of a launch that is nothing but latency.
    const uint32_t my_logical = blockIdx.x * R + lane;
    const bool integrates = wid == 0 && lane < R && my_logical < p.n_recv && p.flags == 0;
    float2 vel0 = make_float2(0.f, 0.f);
    if (integrates) vel0 = p.vel[receiver_slot(p, my_logical)];
    uint32_t open_groups = 0;   // groups of four added since the last block close

    for (uint32_t t = 0; t < ntiles; t++) {
        if (t > 0) __syncthreads();   // every lane is done reading the previous tile
        sxy[tid] = q0;
        sxy[tid + WAVE * W] = q1;
        sgm[tid] = m0;
        sgm[tid + WAVE * W] = m1;
        if (t + 1 < ntiles) fetch(t + 1);   // lands while this tile is being walked
        __syncthreads();

        // this lane's slice of the tile, in whole 8-source granules
        const SourceSlice lane_src = source_slice(min(T, n0 - t * T), 8u, 1, 0, V, v);
        const uint32_t v_lo = lane_src.lo, v_hi = lane_src.hi;

        // Four sources per group: two 16-byte reads of positions, one of G*m (lanes of one lane group read the same
        // address, the groups different ones).  The next group's reads are issued before this group's arithmetic: a
        // lane's slice is a serial chain, and an LDS round trip per four interactions would otherwise sit on it.
        uint32_t j = v_lo;
        const uint32_t groups = (v_hi - v_lo) / 4u;
        v4f P01 = {0.f, 0.f, 0.f, 0.f}, P23 = {0.f, 0.f, 0.f, 0.f}, G4 = {0.f, 0.f, 0.f, 0.f};
        if (groups > 0) {
            P01 = *reinterpret_cast<const v4f *>(&sxy[j]);
            P23 = *reinterpret_cast<const v4f *>(&sxy[j + 2]);
            G4 = *reinterpret_cast<const v4f *>(&sgm[j]);
        }
        for (uint32_t g = 0; g < groups; g++) {
            const v4f A01 = P01, A23 = P23, AG = G4;
            const uint32_t jn = g + 1 < groups ? j + 4 : j;   // the last group re-reads itself instead of branching
            P01 = *reinterpret_cast<const v4f *>(&sxy[jn]);
            P23 = *reinterpret_cast<const v4f *>(&sxy[jn + 2]);
            G4 = *reinterpret_cast<const v4f *>(&sgm[jn]);
            interact<1, false>(Rv, f2v{A01[0], A01[1]}, AG[0]);
            interact<1, false>(Rv, f2v{A01[2], A01[3]}, AG[1]);
            interact<1, false>(Rv, f2v{A23[0], A23[1]}, AG[2]);
            interact<1, false>(Rv, f2v{A23[2], A23[3]}, AG[3]);
            j += 4;
            if (++open_groups == 32) {   // 128 sources: half the classic kernel's block (K = 1 chains round more often)
                Rv.close_chunk();
                open_groups = 0;
            }
        }
        for (; j < v_hi; j++) {
            const float2 a0 = sxy[j];
            interact<1, false>(Rv, f2v{a0.x, a0.y}, sgm[j]);
        }
    }
    Rv.close_chunk();   // whatever is still open (a no-op on exact zeros)

    // W x H partial sums per receiver meet in LDS.  Two levels, fixed order: thread (c, r) of the first wave adds the
    // slices [c * V / S, (c + 1) * V / S) of receiver r, then thread r adds those S sums -- 64 dependent adds by 16
    // threads would be the longest serial chain of a short launch.  Plain adds, like the classic kernel's sum over its W
    // slices and split parts (compensating them measured +0.15 us per step at N = 500 ... 2 000 and bought no accuracy:
    // the error sits in the lanes' own block sums, which is why those close every 128 sources here).
    partial[v * R + r] = make_float2(Rv.s[0].x, Rv.s[0].y);
    __syncthreads();
    constexpr uint32_t S = WAVE / R;        // = H second-level terms per receiver, computed by the first wave's 64 lanes
    constexpr uint32_t PER = V / S;         // = W slices per first-level sum
    if (wid == 0) {
        const uint32_t c = lane / R, rr = lane % R;
        float sx = 0.0f, sy = 0.0f;
#pragma unroll
        for (uint32_t s2 = 0; s2 < PER; s2++) {
            const float2 t = partial[(c * PER + s2) * R + rr];
            sx = __fadd_rn(sx, t.x);
            sy = __fadd_rn(sy, t.y);
        }
        // same wave: LDS executes one wave's accesses in order; the fences only stop the compiler from reordering
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        partial[V * R + lane] = make_float2(sx, sy);   // second-level buffer behind the first: [S][R]
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < R) {
            float ax = 0.0f, ay = 0.0f;
#pragma unroll
            for (uint32_t c2 = 0; c2 < S; c2++) {
                const float2 t = partial[V * R + c2 * R + lane];
                ax = __fadd_rn(ax, t.x);
                ay = __fadd_rn(ay, t.y);
            }
            if (integrates) {
                // finish_receiver with everything it reads already in registers; `integrates` implies flags == 0, so the
                // carry-in (and with it the old acc, passed as zero) and the no-finalize exit fold away
                finish_loaded(p, receiver_slot(p, my_logical), make_float2(ax, ay), make_float2(0.f, 0.f), vel0,
                              make_float2(Rv.p[0].x, Rv.p[0].y), dt);
            } else {
                finish_receiver(p, my_logical, ax, ay, dt);   // chained passes (flags): the general epilogue
            }
        }
    }
}

template <int W, int H>
__global__ __launch_bounds__(WAVE *W) void lane_split_kernel(const StepParams p) {
    lane_split_body<W, H>(p);
}

// ---- the one-workgroup chain -------------------------------------------------------------------------------------
//
// Worlds of a few hundred particles are bound by the kernel boundary, not by arithmetic: at N = 250 a step is 30 000
// interactions -- 1.3 us on ONE compute unit -- while a dependent launch costs 1.6-1.8 us before its kernel has
// loaded anything (profiles/r01_ubench6_launch_floor.txt).  So such a world runs its whole n-step chain inside one
// launch of one 1024-thread workgroup: positions ping-pong between two LDS arrays, G*m sits in LDS, radii and
// velocities stay in registers, and a step is {force loop from LDS, partial sums to LDS, barrier, sum + integrate,
// barrier}.  Nothing crosses the chip per step.  (More than one workgroup would need an in-kernel all-gather of the
// positions per step: 2.4 us for 8 KB between 32 CUs, MI355X_MICROARCH.md price list "allgather" -- dearer than the
// kernel boundary it would replace, which is why the path stops at one workgroup.)
//
// Bit-compatible with the per-step kernel by construction: same interaction statements, same slicing arithmetic
// (granule 8, W = 16 / tiles slices per receiver tile), same block closes, same reduction order, same integrator
// roundings -- tests/test_gpu_parity.py holds it to plain launches of k = 2, w = 16 / tiles, split = 1, unit = 8.
// (the body as a device function: chain_kernel runs it for one world, batch_chain_kernel for one member per workgroup)
//
// TRACE (batch_trace_chain_kernel): the same steps, and after every tr.every-th one the workgroup records the energy sums
// of the state it holds -- positions and G*m are in LDS already, the masses join them at load time, the integrating
// threads drop their velocities there when a record is due -- with the diagnostics' own functions (diag_common.h), so a
// row has the bits of ensemble_phi_kernel + ensemble_reduce_kernel: the first wave of chain tile t IS the wave of
// diagnostics tile t (both hold receivers 128 t + lane and + 64, and it has their radii in registers), the tiles' rows meet
// in LDS, and the first 256 threads add them.  One extra barrier per record; the steps themselves are untouched, and
// without TRACE nothing of this is compiled.  LDS with TRACE: 26 KB of the chain + 6.25 KB, of the workgroup's 160 KB.
struct ChainTrace {
    const float *mass;   // the member's masses
    double *row;         // the member's row of the first record this launch makes
    size_t pitch;        // doubles from one record's row to the next
    uint32_t until;      // steps until the next record
    uint32_t every;
    bool entry;          // record the state on entry
};

template <bool TRACE>
__device__ __forceinline__ void chain_body(const ChainParams &p, const ChainTrace &tr) {
    constexpr int K = CHAIN_K;
    static_assert(CHAIN_K == nbd::K && WAVE * CHAIN_K == nbd::TILE, "a chain tile is a diagnostics tile");
    __shared__ __attribute__((aligned(16))) float spos[2][2 * CHAIN_MAX_RECV];  // (x, y) interleaved, ping-pong
    __shared__ __attribute__((aligned(16))) float sgm[CHAIN_MAX_RECV];
    __shared__ float2 partial[16][WAVE * K];
    __shared__ float smass[TRACE ? CHAIN_MAX_RECV : 1];
    __shared__ float2 svel[TRACE ? CHAIN_MAX_RECV : 1];
    __shared__ double srow[TRACE ? CHAIN_MAX_RECV / (WAVE * K) : 1][nbd::QTY];

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t W = 16u / p.tiles;              // waves (= source slices) per receiver tile
    const uint32_t tile = wid / W, slice = wid % W;
    const uint32_t tile_base = tile * (WAVE * K);
    const float dt = *p.dt;

    // ---- load: every position and G*m into LDS, this lane's radii and (integrating threads) velocity into registers
    for (uint32_t i = tid; i < p.n_recv; i += 1024) {
        const float2 q = p.pos[i];
        spos[0][2 * i] = q.x;
        spos[0][2 * i + 1] = q.y;
        if (i < p.n_src) sgm[i] = p.src_gm[i];
        if constexpr (TRACE)
            if (i < p.n_src) smass[i] = tr.mass[i];
    }
    Receivers<K> R;
    uint32_t ridx[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        uint32_t i = tile_base + k * WAVE + lane;
        i = i < p.n_recv ? i : p.n_recv - 1;  // tail lanes redo the last receiver; they never store
        ridx[k] = i;
        R.r[k] = p.radius[i];
    }
    // the thread that integrates receiver slot `local` of its tile (the per-step kernel's `slot = tid` thread)
    const uint32_t local = tid - tile * W * WAVE;
    const uint32_t mine = tile_base + local;
    const bool integrates = local < WAVE * K && mine < p.n_recv;
    float2 v = make_float2(0.f, 0.f), a = make_float2(0.f, 0.f);
    if (integrates) v = p.vel[mine];

    // this wave's slice of the sources: whole 8-source granules, exactly StepParams::unit = 8 with split = 1
    const SourceSlice wave_src = source_slice(p.n_src, 8u, 1, 0, W, slice);
    const uint32_t v_lo = wave_src.lo, v_hi = wave_src.hi;

    // One record: the state in S / svel -> the member's row.  Every thread of the workgroup calls it.
    double *row = tr.row;
    auto record = [&](const float *S) {
        const uint32_t rb = tile_base;
        if (slice == 0 && rb < p.n_src) {   // the energy sums run over the massive receivers only
            float px[K], py[K];
            uint32_t ri[K];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t i = rb + k * WAVE + lane;
                ri[k] = i < p.n_src ? i : p.n_src - 1;  // tail lanes redo the last receiver; their results are dropped
                px[k] = S[2 * ri[k]];
                py[k] = S[2 * ri[k] + 1];
            }
            // R.r[k] is the radius of receiver min(i, n_recv - 1): that of ri[k] in every live lane
            double sum[K], e[K][nbd::QTY], t[nbd::QTY];
            nbd::tile_potential(sum, px, py, R.r, ri, rb, p.n_src, nbd::LdsSources{S, sgm});
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t i = rb + k * WAVE + lane;
                nbd::energy_terms(e[k], i < p.n_src, -sum[k], smass, reinterpret_cast<const float2 *>(S), svel, i);
            }
            nbd::tile_tree(t, e);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < nbd::QTY; q++) srow[tile][q] = t[q];
            }
        }
        __syncthreads();
        // the next write of srow is a record later, behind the barriers of at least one step
        if (tid < (uint32_t)nbd::REDUCE_THREADS)
            nbd::reduce_rows_shfl(&srow[0][0], (p.n_src + nbd::TILE - 1) / nbd::TILE, row, tid);
        row += tr.pitch;
    };
    uint32_t until = tr.until;
    if constexpr (TRACE)
        if (tr.entry && integrates) svel[mine] = v;
    __syncthreads();
    if constexpr (TRACE)
        if (tr.entry) record(spos[0]);

    int cur = 0;
    for (uint32_t step = 0; step < p.steps; step++) {
        const bool due = TRACE && --until == 0;
        const float *S = spos[cur];
#pragma unroll
        for (int k = 0; k < K; k++) R.p[k] = f2v{S[2 * ridx[k]], S[2 * ridx[k] + 1]};
        R.clear();
        uint32_t j = v_lo;
        const uint32_t groups = (v_hi - v_lo) / 8u;
        for (uint32_t g = 0; g < groups; g++, j += 8) {
            const v16f P = *reinterpret_cast<const v16f *>(&S[2 * j]);   // broadcast reads: every lane the same address
            const v8f G = *reinterpret_cast<const v8f *>(&sgm[j]);
            interact8<K, false>(R, P, G);
            if ((g & (8u * CLOSE_EVERY - 1)) == 8u * CLOSE_EVERY - 1) R.close_chunk();   // every 256 sources of the slice
        }
        for (; j < v_hi; j++) interact<K, false>(R, f2v{S[2 * j], S[2 * j + 1]}, sgm[j]);
        if ((v_hi - v_lo) & (CHUNK * CLOSE_EVERY - 1)) R.close_chunk();                   // a short last block
#pragma unroll
        for (int k = 0; k < K; k++) partial[wid][k * WAVE + lane] = make_float2(R.s[k].x, R.s[k].y);
        __syncthreads();
        if (integrates) {
            a = wave_sum(&partial[tile * W][local], WAVE * K, W);   // the tile's slices in wave order, = the per-step kernel
            float2 q = make_float2(S[2 * mine], S[2 * mine + 1]);
            integrate(a, dt, v, q);
            spos[cur ^ 1][2 * mine] = q.x;
            spos[cur ^ 1][2 * mine + 1] = q.y;
            if constexpr (TRACE)
                if (due) svel[mine] = v;
        }
        __syncthreads();
        cur ^= 1;
        if constexpr (TRACE) {
            if (due) {   // the waves that do not record wait at the record's barrier, then at the next step's
                record(spos[cur]);
                until = tr.every;
            }
        }
    }
    if (integrates && (!TRACE || p.steps > 0)) {   // a traced call of no steps changes nothing
        p.pos[mine] = make_float2(spos[cur][2 * mine], spos[cur][2 * mine + 1]);
        p.vel[mine] = v;
        p.acc[mine] = a;
    }
}

__global__ __launch_bounds__(1024) void chain_kernel(const ChainParams p) { chain_body<false>(p, ChainTrace{}); }

// ---- world ensembles: B independent worlds, of one N or of different ones, in one launch ---------------------------
//
// A single world of N <= 3 000 keeps one (chain) or a handful (lane-split) of the chip's 256 compute units busy; the
// others can only be used by MORE WORLDS.  The kernels below run the bodies above once per member: nothing is
// copied, so member b's bits are those of the same world alone in chain_kernel / lane_split_kernel<W, H>, whatever B,
// its index or its neighbours are.  Layout: member-major SoA, every array [B][stride]; a member's source count and step
// size come from device memory (mass_len[b], dt[b]), so neither is baked into a launch.
//
// A launch finds its members by block index or through a list (kernels.h BatchParams / RaggedParams), and that is ALL the
// two differ in: which member a workgroup steps, how many particles the member has, and how many chain tiles those make.
// member_of answers the three once per parameter type and every kernel below is one template over it.  By list, a launch
// covers one group of a ragged ensemble -- the chain group (N <= 512) or one of the two lane-split shapes; everything a
// body branches on (n_recv, tiles, n_src) stays wave-uniform, so member m runs the instructions and the summation order of
// the same particles as the only member of a uniform ensemble of its size.
__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

struct Member {
    uint32_t index, n, tiles;   // tiles: of the chain (chain_tiles(n), n <= CHAIN_MAX_RECV)
};

// `block`: the workgroup's index among the launch's members (chain: blockIdx.x, lane-split: blockIdx.y)
__device__ __forceinline__ Member member_of(const BatchParams &bp, uint32_t block) { return {block, bp.n_recv, bp.tiles}; }

__device__ __forceinline__ Member member_of(const RaggedParams &rp, uint32_t block) {
    const uint32_t index = uniform_u32(rp.members[block]);
    const uint32_t n = uniform_u32(rp.n_len[index]);
    return {index, n, n <= WAVE * CHAIN_K ? 1u : n <= 2 * WAVE * CHAIN_K ? 2u : 4u};
}

__device__ __forceinline__ ChainParams member_chain(const BatchParams &bp, const Member &m) {
    const size_t base = (size_t)m.index * bp.stride;
    ChainParams p;
    p.pos = bp.pos_in + base;   // updated in place, like the single chain
    p.vel = bp.vel + base;
    p.acc = bp.acc + base;
    p.radius = bp.radius + base;
    p.src_gm = bp.gm + base;
    p.n_recv = m.n;
    p.n_src = uniform_u32(bp.mass_len[m.index]);
    p.steps = bp.steps;
    p.tiles = m.tiles;
    p.dt = bp.dt + m.index;
    return p;
}

template <class P>
__global__ __launch_bounds__(1024) void batch_chain_kernel(const P bp) {
    chain_body<false>(member_chain(bp, member_of(bp, blockIdx.x)), ChainTrace{});
}

template <class P>
__global__ __launch_bounds__(1024) void batch_trace_chain_kernel(const P bp, const TraceParams tp) {
    const Member m = member_of(bp, blockIdx.x);
    ChainTrace tr;
    tr.mass = tp.mass + (size_t)m.index * bp.stride;
    tr.pitch = (size_t)tp.count * nbd::QTY;
    tr.entry = tp.done == 0;
    tr.every = tp.every;
    tr.until = tp.every - tp.done % tp.every;
    // records made before this launch: the one on entry and one per `every` steps done; a row is the member's own index
    tr.row = tp.rows + ((size_t)(tp.done == 0 ? 0u : 1u + tp.done / tp.every) * tp.count + m.index) * nbd::QTY;
    chain_body<true>(member_chain(bp, m), tr);
}

template <int W, int H, class P>
__global__ __launch_bounds__(WAVE *W) void batch_lane_split_kernel(const P bp) {
    const Member m = member_of(bp, blockIdx.y);
    // By list, gridDim.x covers the group's largest member: the workgroups past a smaller member's last receiver leave before
    // the first barrier (blockIdx and n are uniform over the workgroup, so all of it leaves).
    if constexpr (std::is_same_v<P, RaggedParams>)
        if (blockIdx.x * (WAVE / H) >= m.n) return;
    const size_t base = (size_t)m.index * bp.stride;
    // the first mass_len[b] receivers of a member ARE its sources
    const StepParams p = plain_step(bp.pos_in + base, bp.gm + base, uniform_u32(bp.mass_len[m.index]), bp.pos_in + base,
                                    bp.pos_out + base, bp.vel + base, bp.acc + base, bp.radius + base, m.n, bp.dt + m.index, 8);
    lane_split_body<W, H>(p);
}

// ---- kernel entry points -------------------------------------------------------------------------------------------
// One row of a lookup: run-time keys (a, b) == (A, B) select KERNEL<A, B, further template arguments>.
#define NB_CASE(KERNEL, A, B, ...) \
    if (a == A && b == B) return reinterpret_cast<const void *>(&KERNEL<A, B, ##__VA_ARGS__>);

template <int VARIANT>
const void *pick(int a, int b) {   // (k, w)
    // W = 4, 8, 16 are what choose_shape picks from; W = 1 is the shape whose summation order does not depend on
    // how the sources are cut up (one wave walks them all), which the sharded-vs-single bit-equality tests rely on.
    NB_CASE(step_kernel, 1, 1, VARIANT) NB_CASE(step_kernel, 1, 4, VARIANT) NB_CASE(step_kernel, 1, 8, VARIANT) NB_CASE(step_kernel, 1, 16, VARIANT)
    NB_CASE(step_kernel, 2, 1, VARIANT) NB_CASE(step_kernel, 2, 4, VARIANT) NB_CASE(step_kernel, 2, 8, VARIANT) NB_CASE(step_kernel, 2, 16, VARIANT)
#ifdef NB_TUNING_SHAPES
    // never auto-selected (profiles/r01_sweep4_shapes_by_n.txt): built only for shape scans (make TUNING=1)
    NB_CASE(step_kernel, 1, 2, VARIANT) NB_CASE(step_kernel, 2, 2, VARIANT) NB_CASE(step_kernel, 4, 1, VARIANT) NB_CASE(step_kernel, 4, 2, VARIANT)
    NB_CASE(step_kernel, 4, 4, VARIANT) NB_CASE(step_kernel, 4, 8, VARIANT) NB_CASE(step_kernel, 4, 16, VARIANT)
#endif
    return nullptr;
}

const void *pick_fused(int a, int b) {   // (k, w)
    NB_CASE(step_kernel, 1, 4, VARIANT_SMEM, true) NB_CASE(step_kernel, 1, 8, VARIANT_SMEM, true) NB_CASE(step_kernel, 1, 16, VARIANT_SMEM, true)
    NB_CASE(step_kernel, 2, 4, VARIANT_SMEM, true) NB_CASE(step_kernel, 2, 8, VARIANT_SMEM, true) NB_CASE(step_kernel, 2, 16, VARIANT_SMEM, true)
    return nullptr;
}

const void *pick_lane_split(int a, int b) {   // (w, lanes)
    NB_CASE(lane_split_kernel, 4, 2) NB_CASE(lane_split_kernel, 8, 2) NB_CASE(lane_split_kernel, 16, 2) NB_CASE(lane_split_kernel, 4, 4)
    NB_CASE(lane_split_kernel, 8, 4) NB_CASE(lane_split_kernel, 16, 4) NB_CASE(lane_split_kernel, 8, 8) NB_CASE(lane_split_kernel, 16, 8)
    return nullptr;
}

}  // namespace

const void *step_kernel_fn(LaunchShape s) {
    if (s.lanes > 1) return pick_lane_split(s.w, s.lanes);
    return s.variant == VARIANT_SMEM ? pick<VARIANT_SMEM>(s.k, s.w) : pick<VARIANT_LDS>(s.k, s.w);
}

const void *step_kernel_fused_fn(LaunchShape s) {
    if (s.lanes > 1 || s.variant != VARIANT_SMEM) return nullptr;
    return pick_fused(s.k, s.w);
}

const void *dealt_kernel_fn(LaunchShape s) {
    if (s.lanes > 1 || s.variant != VARIANT_SMEM) return nullptr;
    const int a = s.k, b = s.w;
    NB_CASE(dealt_kernel, 1, 16) NB_CASE(dealt_kernel, 2, 16)   // the shapes of large launches (launch_shape.hip deal_rule)
    return nullptr;
}

const void *finish_kernel_fn() { return reinterpret_cast<const void *>(&finish_kernel); }

const void *batch_lane_split_fn(int a, int b, bool listed) {   // (w, lanes)
    // the two shapes batch_lane_shape reaches for 512 < N <= 3 000, for either way of finding the members
    if (listed) {
        NB_CASE(batch_lane_split_kernel, 8, 8, RaggedParams) NB_CASE(batch_lane_split_kernel, 16, 4, RaggedParams)
    } else {
        NB_CASE(batch_lane_split_kernel, 8, 8, BatchParams) NB_CASE(batch_lane_split_kernel, 16, 4, BatchParams)
    }
    return nullptr;
}
#undef NB_CASE

void launch_chain(hipStream_t st, const ChainParams &p) {
    hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(1024), 0, st, p);
}

void launch_batch_chain(hipStream_t st, const RaggedParams &p, uint32_t workgroups) {
    if (p.members)
        hipLaunchKernelGGL(batch_chain_kernel<RaggedParams>, dim3(workgroups), dim3(1024), 0, st, p);
    else
        hipLaunchKernelGGL(batch_chain_kernel<BatchParams>, dim3(workgroups), dim3(1024), 0, st, static_cast<const BatchParams &>(p));
}

void launch_batch_trace_chain(hipStream_t st, const RaggedParams &p, const TraceParams &t, uint32_t workgroups) {
    if (p.members)
        hipLaunchKernelGGL(batch_trace_chain_kernel<RaggedParams>, dim3(workgroups), dim3(1024), 0, st, p, t);
    else
        hipLaunchKernelGGL(batch_trace_chain_kernel<BatchParams>, dim3(workgroups), dim3(1024), 0, st, static_cast<const BatchParams &>(p), t);
}

}  // namespace nb
