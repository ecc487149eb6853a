// diagnostics.hip -- energy, momentum and per-particle potential of the state a pipeline holds (include/nbody_diag.h).
//
// Definitions (also in include/nbody_diag.h and DESIGN.md section 3): particles in the World's partitioned order, M =
// mass_len, G*m_j = src_gm[j] (what the step kernels use), softening = the RECEIVER's radius added to the squared
// distance, not squared (reference sim_cpu.c:173-176):
//     Phi_i = - sum_{j < M, j != i} G*m_j / sqrt(|x_j - x_i|^2 + r_i)        for every receiver i, massless ones included
// The self term is excluded BY INDEX inside the loop (subtracting it afterwards would cancel most of the fp32 digits
// of a galaxy core, where G*m_i / sqrt(r_i) is 10^3..10^4 x the rest of the sum).
//
// potential_kernel: one workgroup = W waves over the same 64 * K receivers (a tile), each wave walks a 1/W slice of the
// sources in blocks of 256 -- the step kernel's scalar-cache route: wave-uniform sources arrive in SGPRs through
// s_load_dwordx16 / x8.  Per (receiver, source) pair:
//     v_sub_f32 dx, v_sub_f32 dy, v_fma_f32 q = dx*dx + r, v_fma(c)_f32 q += dy*dy, v_rsq_f32 t, v_fmac_f32 phi += G*m * t
// = 5 plain VALU + 1 rsq (~18 cycles per wave-interaction against the step kernel's 26).  Only the one source block
// that contains the tile's own indices takes the masked path (a v_cndmask per pair); every other block runs unmasked.
// Sums: plain fp32 over each block of 256 sources, float64 across block totals and across the W waves (fixed order).
// With `slab`, every workgroup also reduces its receivers' float64 terms (m_i Phi_i, m_i |v_i|^2, m_i, m_i v_i,
// m_i (x_i v_y,i - y_i v_x,i), m_i x_i) in a fixed tree and stores them to slab[workgroup]; energy_reduce_kernel then
// adds the slab in a fixed order.  No float atomics anywhere: results are bitwise reproducible from call to call.
//
// The C-ABI entry points nb_hip_energy / nb_hip_potential sit at the bottom of this file.
#include "pipeline_internal.h"
#include "diag_common.h"
#include "nbody_hip_tuning.h"

namespace nbd {
namespace {

struct DiagParams {
    const float2 *pos;     // pos[cur]: the latest state
    const float2 *vel;
    const float *radius;
    const float *mass;
    const float *src_gm;   // G * m_j, j < n_src
    uint32_t n_recv;       // receivers [0, n_recv)
    uint32_t n_src;        // sources [0, n_src) = [0, M)
    float *phi;            // nullable: Phi_i, i < n_recv
    double *slab;          // nullable: QTY doubles per workgroup
};

// the pair statement, the block sum, the eight terms and the row sum: diag_common.h (shared with batch_diag.hip)

// 512 threads, at most 64 VGPRs (8 waves per SIMD: four workgroups per CU).
__global__ __launch_bounds__(WAVE * W, 8) void potential_kernel(const DiagParams p) {
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t rb = blockIdx.x * TILE;  // first receiver of the tile

    float px[K], py[K], r[K], a[K];
    uint32_t ri[K];
    double s[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        uint32_t i = rb + k * WAVE + lane;
        i = i < p.n_recv ? i : p.n_recv - 1;  // tail lanes redo the last receiver; their results are dropped
        const float2 q = p.pos[i];
        px[k] = q.x;
        py[k] = q.y;
        r[k] = p.radius[i];
        ri[k] = i;
        a[k] = 0.0f;
        s[k] = 0.0;
    }

    // this wave's slice of the sources, in whole blocks
    const uint32_t nblocks = (p.n_src + BLOCK - 1) / BLOCK;
    const uint32_t per_wave = (nblocks + W - 1) / W;
    const uint32_t b_lo = min(wid * per_wave, nblocks);
    const uint32_t b_hi = min(b_lo + per_wave, nblocks);
    const ConstF sp = (ConstF)(uintptr_t)p.pos, sg = (ConstF)(uintptr_t)p.src_gm;
    for (uint32_t b = b_lo; b < b_hi; b++) {
        const uint32_t j0 = b * BLOCK, j1 = min(j0 + BLOCK, p.n_src);
        if (j0 < rb + TILE && rb < j1)  // the tile's own indices: the one masked block
            block_sum<true>(a, px, py, r, ri, sp, sg, j0, j1);
        else
            block_sum<false>(a, px, py, r, ri, sp, sg, j0, j1);
#pragma unroll
        for (int k = 0; k < K; k++) {
            s[k] += (double)a[k];
            a[k] = 0.0f;
        }
    }

    // the W slices in wave order (float64), then Phi_i = -sum
    __shared__ double part[W][TILE];
#pragma unroll
    for (int k = 0; k < K; k++) part[wid][k * WAVE + lane] = s[k];
    __syncthreads();
    double e[QTY];
    if (tid < TILE) {
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < W; w++) sum += part[w][tid];
        const double phi = -sum;
        const uint32_t i = rb + tid;
        const bool live = i < p.n_recv;
        if (live && p.phi) p.phi[i] = (float)phi;
        if (p.slab) {
            energy_terms(e, live, phi, p.mass, p.pos, p.vel, i);
        }
    }
    if (!p.slab) return;
    // fixed tree over the tile's receivers, one quantity per row of the reused LDS
    __syncthreads();
    double(*red)[TILE] = part;   // QTY == W rows of TILE
    if (tid < TILE) {
#pragma unroll
        for (int q = 0; q < QTY; q++) red[q][tid] = e[q];
    }
    __syncthreads();
    for (uint32_t half = TILE / 2; half > 0; half /= 2) {
        if (tid < half) {
#pragma unroll
            for (int q = 0; q < QTY; q++) red[q][tid] = red[q][tid] + red[q][tid + half];
        }
        __syncthreads();
    }
    if (tid < QTY) p.slab[(size_t)blockIdx.x * QTY + tid] = red[tid][0];
}
static_assert(QTY == W, "the slab reduction reuses the wave-partial LDS rows");

// One workgroup: out[q] = sum over the slab's rows of quantity q (reduce_rows, diag_common.h).
__global__ __launch_bounds__(REDUCE_THREADS) void energy_reduce_kernel(const double *slab, uint32_t rows, double *out) {
    reduce_rows(slab, rows, out);
}

}  // namespace
}  // namespace nbd

namespace {

using namespace nbi;
using nbd::QTY;

// The state the step kernels will read next: the sources of an unsharded pipeline are its first mass_len receivers.
nbd::DiagParams diag_params(SimPipeline *s, uint32_t n_recv) {
    nbd::DiagParams p{};
    p.pos = s->pos[s->cur];
    p.vel = s->vel;
    p.radius = s->radius;
    p.mass = s->mass;
    p.src_gm = s->src_gm;
    p.n_recv = n_recv;
    p.n_src = s->data.mass_len;
    return p;
}

}  // namespace

namespace nbi {

// shared with field.hip (pipeline_internal.h): the checks of every diagnostic of one pipeline
void check_diag(SimPipeline *s, const char *what) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    NB_ASSERT(!s->sharded, "%s of a sharded pipeline needs a collective over the ranks: not supported", what);
    NB_ASSERT(s->on_device, "%s before SetSimulationData", what);
}

}  // namespace nbi

extern "C" {

void nb_hip_energy(SimPipeline *s, WorldEnergy *out) {
    check_diag(s, "nb_hip_energy");
    NB_ASSERT(out != nullptr, "NULL WorldEnergy");
    const uint32_t M = s->data.mass_len;
    double q[QTY] = {0};
    if (M > 0) {
        const uint32_t rows = (M + nbd::TILE - 1) / nbd::TILE;
        // the float64 slab: QTY per workgroup + the QTY results
        read_call(s, s->read.iv, "nb_hip_energy", nullptr, 0, (size_t)(rows + 1) * QTY * sizeof(double), q, sizeof(q), [&](void *, void *work) -> const void * {
            double *slab = static_cast<double *>(work);
            nbd::DiagParams p = diag_params(s, M);
            p.slab = slab;
            hipLaunchKernelGGL(nbd::potential_kernel, dim3(rows), dim3(nbd::WAVE * nbd::W), 0, s->stream, p);
            ASSERT_HIP(hipGetLastError(), "potential_kernel launch (energy, %u receivers)", M);
            double *res = slab + (size_t)rows * QTY;
            hipLaunchKernelGGL(nbd::energy_reduce_kernel, dim3(1), dim3(nbd::REDUCE_THREADS), 0, s->stream, slab, rows, res);
            ASSERT_HIP(hipGetLastError(), "energy_reduce_kernel launch");
            return res;
        });
    } else {
        s->read.iv.clear();
    }
    nb_energy_from_sums(q, out);
}

void nb_hip_potential(SimPipeline *s, float *phi) {
    check_diag(s, "nb_hip_potential");
    const uint32_t N = s->data.total_len;
    NB_ASSERT(phi != nullptr || N == 0, "NULL phi");
    if (N == 0) {
        s->read.iv.clear();
        return;
    }
    const size_t bytes = (size_t)N * sizeof(float);
    read_call(s, s->read.iv, "nb_hip_potential", nullptr, 0, bytes, phi, bytes, [&](void *, void *work) -> const void * {
        nbd::DiagParams p = diag_params(s, N);
        p.phi = static_cast<float *>(work);
        hipLaunchKernelGGL(nbd::potential_kernel, dim3((N + nbd::TILE - 1) / nbd::TILE), dim3(nbd::WAVE * nbd::W), 0, s->stream, p);
        ASSERT_HIP(hipGetLastError(), "potential_kernel launch (%u receivers)", N);
        return work;
    });
}

// tuning hook (nbody_hip_tuning.h): device time of the kernels of the last read-only call (pipeline_internal.h read_call)
double nb_hip_last_diag_ms(SimPipeline *s) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    if (!s->read.iv.valid()) return 0.0;
    use_device();
    return s->read.iv.ms();
}

}  // extern "C"
