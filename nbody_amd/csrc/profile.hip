// profile.hip -- radial profiles of the state a pipeline or an ensemble holds (include/nbody_profile.h): the six float64
// annulus moments per row, nb_hip_profile and nb_hip_ensemble_profile of include/nbody_hip.h.
//
// The statement (one particle's terms, the row of a squared radius) is profile_common.h, shared with the host path.  What is
// written here is the ORDER, which is the contract: chunks of 1024 consecutive particles, inside a chunk every row's terms in
// index order from +0.0, then the chunk totals in chunk order from +0.0.
//
// chunk_rows, one 256-thread workgroup over one chunk:
//   stage   thread t evaluates particles t, t + 256, t + 512, t + 768 of the chunk (coalesced float2 loads), finds each row by
//           binary search over e2[] in LDS and stores the row (uint16) and the five terms (float64, one array per term: lane-
//           consecutive 8-byte slots, no bank conflict) at the particle's slot
//   count   the 256 threads are G pieces x P rows (P = rows rounded up to 64, 128 or 256; G = 256 / P = 4, 2 or 1 whole waves or
//           wave pairs): thread (g, r) counts the slots of row r in the g-th G-th of the chunk.  All lanes of a wave read the same
//           16 bytes of row[] (a broadcast), eight slots per ds_read_b128, no branch
//   scan    exclusive prefix of the 256 counts in the order (row, piece) (wave shuffles + four wave totals): row r's pieces lie
//           side by side in slot order, so the prefix is where each piece's part of row r's list starts
//   list    thread (g, r) walks its piece again and writes the matching slots, ascending, from its start on: a stable rank from
//           integer counts.  Branch-free: a slot that does not match is stored to the thread's own spare entry behind the list
//   sum     thread (0, r) adds row r's entries in list order.  Lanes walk lists of different length side by side: a wave takes
//           as long as its fullest row, not as the sum of its rows (which a conditional add inside the count would)
// Integer LDS atomics count the NaN particles (an integer sum has no order); there is no float atomic anywhere.
//
// profile_chunk_kernel stores every chunk's rows x 6 totals (and its NaN count) to a slab; profile_reduce_kernel adds the slab's
// chunks in order, one thread per cell, fed from LDS tiles its workgroup loads together.  ensemble_profile_kernel is one workgroup per member, uniform or ragged: it walks
// the member's three chunks or fewer with the same chunk_rows, adds the totals in registers in chunk order and stores the
// final rows, so member b is bit for bit nb_hip_profile of the same particles.
//
// LDS per workgroup: 1024 x (2 + 2 + 40) B of slots, 256 x (8 + 2 + 8) B of edges, spare entries and counts: 49 696 B = 48.5 KiB
// (three workgroups per CU).
#include "batch_internal.h"
#include "profile_common.h"

namespace nb {
namespace profile {
namespace {

constexpr uint32_t CHUNK = NB_PROFILE_CHUNK, THREADS = 256, PER_THREAD = CHUNK / THREADS, WAVE = 64;
constexpr uint32_t QTY = NB_PROFILE_QTY, TERMS = NB_PROFILE_TERMS, ROWS_MAX = NB_PROFILE_MAX_BINS + 2;
constexpr uint32_t ABSENT = 0xfffeu;   // a slot past the last particle: in no row and not unplaced either
static_assert(ROWS_MAX <= THREADS, "one thread per row");
static_assert(CHUNK % (8 * 4) == 0 && CHUNK % THREADS == 0 && CHUNK <= ABSENT, "slots are uint16, read eight at a time, in up to four pieces");

struct Stage {
    double term[TERMS][CHUNK];
    uint16_t row[CHUNK] __attribute__((aligned(16)));
    uint16_t list[CHUNK + THREADS];   // the rows' lists back to back, then one spare entry per thread
    double e2[ROWS_MAX];
    uint32_t count[THREADS], start[THREADS];   // per (row, piece), in that order
    uint32_t wave_total[THREADS / WAVE];
    uint32_t lost;
};

// the particles a launch reads: [0, n) of these arrays
struct Source {
    const float2 *pos;
    const float2 *vel;
    const float *mass;
    uint32_t n;
};

// What every kernel starts with: e2[] from the uploaded edges, the NaN counter at 0.  Followed by a barrier.
__device__ __forceinline__ void stage_edges(Stage &st, const float *edges, uint32_t bins) {
    if (threadIdx.x <= bins) st.e2[threadIdx.x] = nb_profile_edge2(edges[threadIdx.x]);
    if (threadIdx.x == 0) st.lost = 0;
    __syncthreads();
}

// calls f(slot, is it of row r) for every slot of [lo, hi), ascending; lo and hi are multiples of 8
template <class F>
__device__ __forceinline__ void for_slots(const Stage &st, uint32_t lo, uint32_t hi, uint32_t r, F f) {
    const uint4 *rows8 = reinterpret_cast<const uint4 *>(st.row);
    for (uint32_t s = lo; s < hi; s += 8) {
        const uint4 v = rows8[s / 8];
        f(s, (v.x & 0xffffu) == r);
        f(s + 1, (v.x >> 16) == r);
        f(s + 2, (v.y & 0xffffu) == r);
        f(s + 3, (v.y >> 16) == r);
        f(s + 4, (v.z & 0xffffu) == r);
        f(s + 5, (v.z >> 16) == r);
        f(s + 6, (v.w & 0xffffu) == r);
        f(s + 7, (v.w >> 16) == r);
    }
}

// The chunk [first, first + CHUNK) of src: thread r < bins + 2 leaves with tot[] = the chunk's six totals of row r (every other
// thread with zeros).  Called by all 256 threads, first < src.n; ends in a barrier, so it can be called again at once.
__device__ __forceinline__ void chunk_rows(Stage &st, const Source &src, uint32_t first, uint32_t bins, const float *centre, bool by_mass,
                                           double *tot) {
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE, rows = bins + 2;
#pragma unroll
    for (uint32_t k = 0; k < PER_THREAD; k++) {
        const uint32_t slot = k * THREADS + tid, i = first + slot;
        double term[TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
        uint32_t r = ABSENT;
        if (i < src.n) {
            const float2 p = src.pos[i], v = src.vel[i];
            const double wgt = by_mass ? (double)src.mass[i] : 1.0;
            const double q = nb_profile_terms(p.x, p.y, v.x, v.y, wgt, centre, term);
            r = nb_profile_row(st.e2, bins, q);
            if (r == NB_PROFILE_UNPLACED) atomicAdd(&st.lost, 1u);
        }
        st.row[slot] = (uint16_t)r;
#pragma unroll
        for (uint32_t c = 0; c < TERMS; c++) st.term[c][slot] = term[c];
    }

    // thread (g, r): piece g of row r; a piece is CHUNK / G slots, cut at the last live slot (those past it are ABSENT)
    const uint32_t shift = rows <= 64 ? 6 : rows <= 128 ? 7 : 8;   // log2 P
    const uint32_t pieces = THREADS >> shift, g = tid >> shift, r = tid & ((1u << shift) - 1), at_table = r * pieces + g;
    const uint32_t left = src.n - first;
    const uint32_t live = left < CHUNK ? (left + 7u) & ~7u : CHUNK;
    const uint32_t piece = CHUNK / pieces, lo = min(g * piece, live), hi = min(lo + piece, live);
    __syncthreads();
    uint32_t cnt = 0;
    if (r < rows) for_slots(st, lo, hi, r, [&](uint32_t, bool mine) { cnt += mine; });
    st.count[at_table] = cnt;
    __syncthreads();

    const uint32_t own = st.count[tid];
    uint32_t upto = own;   // inclusive prefix inside the wave
#pragma unroll
    for (uint32_t d = 1; d < WAVE; d *= 2) {
        const uint32_t below = __shfl_up(upto, d);
        if (lane >= d) upto += below;
    }
    if (lane == WAVE - 1) st.wave_total[wid] = upto;
    __syncthreads();
    uint32_t before = upto - own;
    for (uint32_t w = 0; w < wid; w++) before += st.wave_total[w];
    st.start[tid] = before;
    __syncthreads();

    if (r < rows) {
        uint32_t at = st.start[at_table];
        const uint32_t spare = CHUNK + tid;
        for_slots(st, lo, hi, r, [&](uint32_t slot, bool mine) {
            st.list[mine ? at : spare] = (uint16_t)slot;
            at += mine;
        });
    }
    __syncthreads();

#pragma unroll
    for (uint32_t c = 0; c < QTY; c++) tot[c] = 0.0;
    if (tid < rows) {   // piece 0 of row tid: the row's whole list starts where its first piece does
        const uint32_t begin = st.start[tid * pieces];
        uint32_t total = 0;
        for (uint32_t k = 0; k < pieces; k++) total += st.count[tid * pieces + k];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
        for (uint32_t a = begin; a < begin + total; a++) {
            const uint32_t slot = st.list[a];
            s0 += st.term[0][slot];
            s1 += st.term[1][slot];
            s2 += st.term[2][slot];
            s3 += st.term[3][slot];
            s4 += st.term[4][slot];
        }
        tot[0] = (double)total;
        tot[1] = s0;
        tot[2] = s1;
        tot[3] = s2;
        tot[4] = s3;
        tot[5] = s4;
    }
    __syncthreads();
}

struct ChunkParams {
    Source src;
    const float *in;   // bins + 1 edges, then the centre's four floats
    uint32_t bins;
    int by_mass;
    double *slab;      // [chunks][rows * QTY + 1]: the chunk's rows, then its NaN count
};

// One workgroup per chunk of 1024 particles.
__global__ __launch_bounds__(THREADS) void profile_chunk_kernel(const ChunkParams p) {
    __shared__ Stage st;
    stage_edges(st, p.in, p.bins);
    const float *c = p.in + p.bins + 1;
    const float centre[4] = {c[0], c[1], c[2], c[3]};
    const Source src = p.src;   // a copy: a reference to the by-value kernel argument would cost its pointers their address space
    double tot[QTY];
    chunk_rows(st, src, blockIdx.x * CHUNK, p.bins, centre, p.by_mass != 0, tot);
    const uint32_t rows = p.bins + 2;
    double *mine = p.slab + (size_t)blockIdx.x * (rows * QTY + 1);
    if (threadIdx.x < rows) {
#pragma unroll
        for (uint32_t q = 0; q < QTY; q++) mine[threadIdx.x * QTY + q] = tot[q];
    }
    if (threadIdx.x == 0) mine[rows * QTY] = (double)st.lost;
}

// out[i] = cell i of the slab's chunks added in chunk order from +0.0; the last cell, the NaN count, leaves as uint32.  The sum of
// a cell is sequential by contract, so what a workgroup buys is the loads: it owns 8 adjacent cells (64 bytes of every slab row),
// all 256 threads bring 256 chunks x 8 cells to LDS at once, then thread c < 8 goes on with cell c's sum from LDS.
constexpr uint32_t RED_CELLS = 8, RED_ROWS = 256;
__global__ __launch_bounds__(THREADS) void profile_reduce_kernel(const double *slab, uint32_t chunks, uint32_t cells, double *out) {
    __shared__ double tile[RED_ROWS][RED_CELLS];
    const uint32_t tid = threadIdx.x, c = tid % RED_CELLS, r0 = tid / RED_CELLS;
    const uint32_t cell = blockIdx.x * RED_CELLS + c;   // cells + 1 values per chunk: cell <= cells is one of them
    const size_t stride = (size_t)cells + 1;
    double sum = 0.0;
    for (uint32_t base = 0; base < chunks; base += RED_ROWS) {
#pragma unroll
        for (uint32_t k = 0; k < RED_ROWS * RED_CELLS / THREADS; k++) {
            const uint32_t row = k * (THREADS / RED_CELLS) + r0, ch = base + row;
            tile[row][c] = ch < chunks && cell <= cells ? slab[(size_t)ch * stride + cell] : 0.0;
        }
        __syncthreads();
        if (tid < RED_CELLS) {
            const uint32_t n = min(RED_ROWS, chunks - base);
            for (uint32_t row = 0; row < n; row++) sum += tile[row][tid];
        }
        __syncthreads();
    }
    if (tid < RED_CELLS && cell <= cells) {
        if (cell < cells)
            out[cell] = sum;
        else
            *reinterpret_cast<uint32_t *>(out + cells) = (uint32_t)sum;
    }
}

struct EnsembleParams {
    const float2 *pos;          // the SoA arrays of a SimBatch: member b's rows start at b * stride
    const float2 *vel;
    const float *mass;
    const uint32_t *mass_len;   // [count]
    const uint32_t *n_len;      // [count] of a ragged ensemble, else null: every member has n particles
    uint32_t n, stride;
    const float *in;            // bins + 1 edges, then [count][4] centres
    uint32_t bins;
    int by_mass;
    double *out;                // [count][rows][QTY]
    uint32_t *lost;             // [count]
};

// One workgroup per member: its chunks one after another, the totals added in chunk order.
__global__ __launch_bounds__(THREADS) void ensemble_profile_kernel(const EnsembleParams p) {
    __shared__ Stage st;
    const uint32_t member = blockIdx.x, rows = p.bins + 2;
    stage_edges(st, p.in, p.bins);
    const float *c = p.in + p.bins + 1 + (size_t)member * 4;
    const float centre[4] = {c[0], c[1], c[2], c[3]};
    const size_t base = (size_t)member * p.stride;
    Source src;
    src.pos = p.pos + base;
    src.vel = p.vel + base;
    src.mass = p.mass + base;
    src.n = p.by_mass ? p.mass_len[member] : (p.n_len ? p.n_len[member] : p.n);
    double sum[QTY] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t first = 0; first < src.n; first += CHUNK) {
        double tot[QTY];
        chunk_rows(st, src, first, p.bins, centre, p.by_mass != 0, tot);
#pragma unroll
        for (uint32_t q = 0; q < QTY; q++) sum[q] += tot[q];
    }
    if (threadIdx.x < rows) {
        double *mine = p.out + ((size_t)member * rows + threadIdx.x) * QTY;
#pragma unroll
        for (uint32_t q = 0; q < QTY; q++) mine[q] = sum[q];
    }
    if (threadIdx.x == 0) p.lost[member] = st.lost;
}

}  // namespace
}  // namespace profile
}  // namespace nb

namespace {

using namespace nbi;
namespace pf = nb::profile;
using pf::CHUNK;
using pf::QTY;
using pf::THREADS;

// what both calls check of their arguments, before anything touches a device
void check_profile(const char *what, const float *edges, uint32_t bins, const float *centres, uint32_t count, int weights, const double *out) {
    NB_ASSERT(edges != nullptr && centres != nullptr && out != nullptr, "%s: NULL argument", what);
    const char *fault = nb_profile_fault(edges, bins, centres, count, weights);
    NB_ASSERT(fault == nullptr, "%s: %s (bins %u, weights %d)", what, fault, bins, weights);
}

}  // namespace

extern "C" {

void nb_hip_profile(SimPipeline *s, const float *edges, uint32_t bins, const float *centre, int weights, double *out, uint32_t *unplaced) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    check_profile("nb_hip_profile", edges, bins, centre, 1, weights, out);
    check_diag(s, "nb_hip_profile");
    const uint32_t rows = bins + 2, cells = rows * QTY;
    const uint32_t n = weights == NB_PROFILE_BY_MASS ? s->data.mass_len : s->data.total_len;
    if (n == 0) {
        for (uint32_t i = 0; i < cells; i++) out[i] = 0.0;
        if (unplaced) *unplaced = 0;
        s->read.iv.clear();
        return;
    }
    const uint32_t chunks = (n + CHUNK - 1) / CHUNK;
    float in[NB_PROFILE_MAX_BINS + 1 + 4];
    memcpy(in, edges, (size_t)(bins + 1) * sizeof(float));
    memcpy(in + bins + 1, centre, 4 * sizeof(float));
    // the float64 slab: a row of cells + 1 per chunk, then the results -- the cells, then the uint32 NaN count
    const size_t row_bytes = (size_t)(cells + 1) * sizeof(double), back_bytes = (size_t)cells * sizeof(double) + sizeof(uint32_t);
    const void *host = read_call(s, s->read.iv, "nb_hip_profile", in, (size_t)(bins + 5) * sizeof(float), (chunks + 1) * row_bytes, nullptr, back_bytes,
                                 [&](void *in_dev, void *work) -> const void * {
        pf::ChunkParams p{};
        p.src.pos = s->pos[s->cur];
        p.src.vel = s->vel;
        p.src.mass = s->mass;
        p.src.n = n;
        p.in = static_cast<const float *>(in_dev);
        p.bins = bins;
        p.by_mass = weights == NB_PROFILE_BY_MASS;
        p.slab = static_cast<double *>(work);
        double *res = p.slab + (size_t)chunks * (cells + 1);
        hipLaunchKernelGGL(pf::profile_chunk_kernel, dim3(chunks), dim3(THREADS), 0, s->stream, p);
        ASSERT_HIP(hipGetLastError(), "profile_chunk_kernel launch (%u particles, %u bins)", n, bins);
        hipLaunchKernelGGL(pf::profile_reduce_kernel, dim3((cells + pf::RED_CELLS) / pf::RED_CELLS), dim3(THREADS), 0, s->stream, p.slab, chunks,
                           cells, res);
        ASSERT_HIP(hipGetLastError(), "profile_reduce_kernel launch (%u chunks)", chunks);
        return res;
    });
    memcpy(out, host, (size_t)cells * sizeof(double));
    if (unplaced) memcpy(unplaced, static_cast<const double *>(host) + cells, sizeof(uint32_t));
}

void nb_hip_ensemble_profile(SimBatch *s, const float *edges, uint32_t bins, const float *centres, int weights, double *out,
                             uint32_t *unplaced) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    check_profile("nb_hip_ensemble_profile", edges, bins, centres, s->count, weights, out);
    NB_ASSERT(s->has_data, "nb_hip_ensemble_profile before nb_hip_batch_set_data");
    const uint32_t rows = bins + 2, count = s->count;
    const size_t cells = (size_t)count * rows * QTY;
    std::vector<float> in(bins + 1 + (size_t)count * 4);
    memcpy(in.data(), edges, (size_t)(bins + 1) * sizeof(float));
    memcpy(in.data() + bins + 1, centres, (size_t)count * 4 * sizeof(float));
    // [count][rows][QTY] float64, then the [count] uint32 NaN counts: the same bytes on the device and on the host
    const size_t bytes = cells * sizeof(double) + (size_t)count * sizeof(uint32_t);
    const void *host = read_call(s, s->read.iv, "nb_hip_ensemble_profile", in.data(), in.size() * sizeof(float), bytes, nullptr, bytes,
                                 [&](void *in_dev, void *work) -> const void * {
        pf::EnsembleParams p{};
        p.pos = s->pos[s->cur];
        p.vel = s->vel;
        p.mass = s->mass;
        p.mass_len = s->mass_len_dev;
        p.n_len = s->n_len_dev;   // null in a uniform ensemble
        p.n = s->n;
        p.stride = s->stride;
        p.in = static_cast<const float *>(in_dev);
        p.bins = bins;
        p.by_mass = weights == NB_PROFILE_BY_MASS;
        p.out = static_cast<double *>(work);
        p.lost = reinterpret_cast<uint32_t *>(p.out + cells);
        hipLaunchKernelGGL(pf::ensemble_profile_kernel, dim3(count), dim3(THREADS), 0, s->stream, p);
        ASSERT_HIP(hipGetLastError(), "ensemble_profile_kernel launch (%u members of %u, %u bins)", count, s->n, bins);
        return work;
    });
    memcpy(out, host, cells * sizeof(double));
    if (unplaced) memcpy(unplaced, static_cast<const double *>(host) + cells, (size_t)count * sizeof(uint32_t));
}

}  // extern "C"
