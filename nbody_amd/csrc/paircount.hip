// paircount.hip -- pair-separation counts of the state a pipeline or an ensemble holds (include/nbody_paircount.h): how many
// pairs fall in every row of the caller's radii, per class of pair, nb_hip_pair_counts and nb_hip_ensemble_pair_counts of
// include/nbody_hip.h.
//
// The statement (q of a pair, the thresholds, the row of a q) is paircount_common.h, shared with the host path.  The result is
// a table of integers, so there is no order to keep: counts meet through integer atomics and the table is still a function of
// the state and the arguments alone.  There is no float atomic.
//
// pair_count_kernel, one launch for a pipeline (count = 1) and for all members of an ensemble, uniform or ragged.  A workgroup
// of W = 8 waves owns one tile of 64 * K = 128 receivers of one class of one member and one span of that class's sources:
//   classes   MM: receivers and sources [0, M), j > i.  TT: both [M, N), j > i.  MT: a rectangle, the larger side as receivers
//             (more tiles), the smaller as sources.  A class not asked for returns at once: its particles are never read
//   tiles     and source blocks of 256 are cut in ABSOLUTE index, so a tile lies inside one block: in a triangular class a tile
//             walks the blocks from its own upwards, and only that first (diagonal) block takes the j > i mask
//   sources   each wave walks 1 / W of the span's blocks; wave-uniform sources arrive through the scalar cache, 8 per
//             s_load_dwordx16 (loads only), single ones up to the first multiple of 8 and after the last
//   pair      v_sub, v_sub, v_mul, v_mul, v_add (the TU builds with -ffp-contract=off: no fma forms q), the 8 x K = 16 pairs of a
//             fetch together.  Then one wave-uniform test on their bit patterns: all q of the wave below the first threshold, or
//             all at or beyond the last -> popcounts added to a scalar, nothing else.  Otherwise pair by pair: the lanes below
//             the first threshold and those at or beyond the last are popcounts too, and only lanes in between run the
//             branch-free search of paircount_common.h over the thresholds in LDS (log2(2 top) <= 8 steps) -- the 16 searches
//             side by side when half of the pairs or more have such lanes, one by one and only those pairs when fewer do; a
//             NaN q goes to the unplaced slot
//   count     uint32 tables per wave in LDS.  Lanes of one row are merged first: while the leading lane's row is shared by
//             MERGE_MIN lanes or more, one lane adds their popcount (all particles coincident: one add per pair of a wave
//             instead of 64 serialised ones); the rest add 1 each, non-returning ds_add_u32
//   flush     thread t adds row t of the W tables in uint64 and, where it is not zero, adds it to the member's table in
//             global memory with one 64-bit integer atomic.  The host zeroes that table in the stream before the launch
//
// The 32-bit bound.  A wave's LDS counter and its two scalar counters receive at most one count per (receiver of the tile,
// source of the span): TILE * SPAN_BLOCKS * BLOCK = 128 * 2^20 = 2^27 < 2^32 between the zeroing and the flush of a workgroup
// (static_assert below); longer source ranges are further spans, grid.y.
//
// Registers: pair_count_kernel at most 72 VGPRs (68 as built: seven waves per SIMD, so three workgroups of eight waves per CU;
// forced under 64 it spills 24 bytes; tests/test_paircount_cpu.py holds the build to the number stated here), no scratch.
// LDS: 8 x 257 x 4 B of tables + 1 KiB of thresholds = 9.0 KiB per workgroup.
#include "batch_internal.h"
#include "paircount_common.h"

namespace nb {
namespace paircount {
namespace {

constexpr uint32_t WAVE = 64, K = 2, TILE = WAVE * K, W = 8, THREADS = WAVE * W, BLOCK = 256;
constexpr uint32_t SPAN_BLOCKS = 4096;                 // source blocks of one workgroup
constexpr uint32_t SLOTS = NB_PAIRS_MAX_BINS + 3;      // rows 0 .. 255, then the unplaced pairs
constexpr uint32_t UNPLACED = SLOTS - 1;
constexpr uint32_t MERGE_MIN = 8;                      // lanes of one row worth one merged add
static_assert((uint64_t)TILE * SPAN_BLOCKS * BLOCK < (1ull << 32), "a 32-bit counter takes at most tile x sources-per-flush counts");
static_assert(BLOCK % TILE == 0 && SLOTS <= THREADS && NB_PAIRS_TABLE <= THREADS, "a tile lies in one block; one thread per row and per threshold");

typedef float v16f __attribute__((ext_vector_type(16)));
typedef const float __attribute__((address_space(4))) *ConstF;   // read-only for the whole launch: scalar loads

struct Params {
    const float2 *pos;          // the latest positions; member b's rows start at b * stride
    const uint32_t *mass_len;   // [count] of an ensemble, else null: m
    const uint32_t *n_len;      // [count] of a ragged ensemble, else null: n
    uint32_t n, m, stride;
    uint32_t classes, bins, top;
    uint32_t tiles;             // grid.x slots per class and member
    float c_first, c_last;      // tab[0], tab[bins]
    unsigned long long *out;    // [count][bins + 3][3], zeroed: the rows, then the unplaced pairs
    float tab[NB_PAIRS_TABLE];  // nb_pair_thresholds
};

struct Counters {
    uint32_t *hist;         // this wave's table
    const float *tab;
    uint32_t top, lane;
    float c_first, c_last;
    uint32_t n_first, n_last;   // wave-uniform: the pairs of rows 0 and bins + 1 that whole waves put there
};

// `valid` lanes add one count to `row` of the wave's table, lanes of one row merged first
__device__ __forceinline__ void add(Counters &c, uint32_t row, bool valid) {
    uint64_t rem = __ballot(valid);
    while (rem) {
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)rem) - 1;
        const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)row, (int)leader);
        const uint64_t group = __ballot(row == r) & rem;
        const uint32_t size = __popcll(group);
        if (size < MERGE_MIN) break;
        if (c.lane == leader) atomicAdd(c.hist + r, size);
        rem &= ~group;
    }
    if ((rem >> c.lane) & 1) atomicAdd(c.hist + row, 1u);
}

// S wave-uniform sources j .. j + S - 1 against the lane's K receivers; MASK: only j > i counts (the diagonal block)
template <bool MASK, uint32_t S>
__device__ __forceinline__ void group(Counters &c, const float (&px)[K], const float (&py)[K], const uint32_t (&ri)[K], const bool (&live)[K],
                                      const float (&sx)[S], const float (&sy)[S], uint32_t j) {
    // A q is +0 or above, +inf or NaN, so its bit pattern orders like its value, with every NaN (either sign) above +inf: two
    // integer min / max per pair tell whether all of the lane's q lie below the first threshold or all at or beyond the last.
    // Pairs that do not count (idle lanes, j <= i) are in the min and max too: that can only send a wave the long way round.
    float q[S][K];
    bool valid[S][K];
    uint32_t lowest = 0xffffffffu, highest = 0;
#pragma unroll
    for (uint32_t u = 0; u < S; u++) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            q[u][k] = nb_pair_q(px[k], py[k], sx[u], sy[u]);
            valid[u][k] = live[k] && (!MASK || j + u > ri[k]);
            lowest = min(lowest, __float_as_uint(q[u][k]));
            highest = max(highest, __float_as_uint(q[u][k]));
        }
    }
    const bool first = __ballot(highest >= __float_as_uint(c.c_first)) == 0;
    const bool last = !first && __ballot(lowest < __float_as_uint(c.c_last) || highest > 0x7f800000u) == 0;
    if (first || last) {   // the whole wave in row 0, or in row bins + 1: popcounts into a scalar
        uint32_t pairs = 0;
#pragma unroll
        for (uint32_t u = 0; u < S; u++) {
#pragma unroll
            for (uint32_t k = 0; k < K; k++) pairs += __popcll(__ballot(valid[u][k]));
        }
        if (first)
            c.n_first += pairs;
        else
            c.n_last += pairs;
        return;
    }
    // Per pair: the lanes below the first threshold and those at or beyond the last are popcounts into the two scalars; only the
    // lanes in between (or with a NaN) are searched and add to the table.
    bool between[S][K];
    uint32_t crowded = 0;   // pairs that have such lanes
#pragma unroll
    for (uint32_t u = 0; u < S; u++) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            const bool below = valid[u][k] && q[u][k] < c.c_first, beyond = valid[u][k] && q[u][k] >= c.c_last;
            c.n_first += __popcll(__ballot(below));
            c.n_last += __popcll(__ballot(beyond));
            between[u][k] = valid[u][k] && !below && !beyond;
            crowded += __ballot(between[u][k]) != 0;
        }
    }
    if (crowded == 0) return;
    if (2 * crowded >= S * K) {
        // most pairs need the search: all S * K side by side, so that a step's LDS reads are independent of one another and only
        // the steps form a chain (measured at N = 2^20, edges across the system: 269 cycles per wave-pair against 363 one by one)
        uint32_t pos[S][K];
#pragma unroll
        for (uint32_t u = 0; u < S; u++) {
#pragma unroll
            for (uint32_t k = 0; k < K; k++) pos[u][k] = 0;
        }
        for (uint32_t step = c.top; step > 0; step /= 2) {   // nb_pair_row_f32, S * K of them
#pragma unroll
            for (uint32_t u = 0; u < S; u++) {
#pragma unroll
                for (uint32_t k = 0; k < K; k++) pos[u][k] = nb_pair_step_f32(c.tab, pos[u][k], step, q[u][k]);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < S; u++) {
#pragma unroll
            for (uint32_t k = 0; k < K; k++) add(c, q[u][k] != q[u][k] ? UNPLACED : pos[u][k], between[u][k]);
        }
    } else {
        // few do (the last edge at 1 % of the system size: 75 cycles per wave-pair against 145 with every search run): one by one
#pragma unroll
        for (uint32_t u = 0; u < S; u++) {
#pragma unroll
            for (uint32_t k = 0; k < K; k++) {
                if (__ballot(between[u][k]) == 0) continue;
                add(c, q[u][k] != q[u][k] ? UNPLACED : nb_pair_row_f32(c.tab, c.top, q[u][k]), between[u][k]);
            }
        }
    }
}

// the sources [j0, j1) of one block
template <bool MASK>
__device__ __forceinline__ void block_pairs(Counters &c, const float (&px)[K], const float (&py)[K], const uint32_t (&ri)[K],
                                            const bool (&live)[K], ConstF sp, uint32_t j0, uint32_t j1) {
    auto one = [&](uint32_t j) {
        const float sx[1] = {sp[2 * (size_t)j]}, sy[1] = {sp[2 * (size_t)j + 1]};
        group<MASK, 1>(c, px, py, ri, live, sx, sy, j);
    };
    uint32_t j = j0;
    for (; j < j1 && (j & 7u); j++) one(j);
    for (; j + 8 <= j1; j += 8) {
        const v16f P = *(const v16f __attribute__((address_space(4))) *)(sp + 2 * (size_t)j);
        float sx[8], sy[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) sx[u] = P[2 * u], sy[u] = P[2 * u + 1];
        group<MASK, 8>(c, px, py, ri, live, sx, sy, j);
    }
    for (; j < j1; j++) one(j);
}

__global__ __launch_bounds__(THREADS) void pair_count_kernel(const Params p) {
    __shared__ uint32_t hist[W][SLOTS];
    __shared__ float tab[NB_PAIRS_TABLE + 1];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const uint32_t per_member = 3 * p.tiles, member = blockIdx.x / per_member, slot = blockIdx.x % per_member;
    const uint32_t cls = slot / p.tiles, tile = slot % p.tiles;
    if (!((p.classes >> cls) & 1u)) return;
    // the same for every lane, and said so: a loaded value would otherwise count as divergent and take the sources off the scalar cache
    const uint32_t n = __builtin_amdgcn_readfirstlane(p.n_len ? p.n_len[member] : p.n);
    const uint32_t m = __builtin_amdgcn_readfirstlane(p.mass_len ? p.mass_len[member] : p.m);
    uint32_t r0, r1, s0, s1;   // receivers [r0, r1), sources [s0, s1)
    const bool tri = cls != 1;
    if (cls == 0) {
        r0 = s0 = 0, r1 = s1 = m;
    } else if (cls == 2) {
        r0 = s0 = m, r1 = s1 = n;
    } else if (n - m > m) {
        r0 = m, r1 = n, s0 = 0, s1 = m;
    } else {
        r0 = 0, r1 = m, s0 = m, s1 = n;
    }
    if (r1 <= r0 || s1 <= s0) return;
    const uint64_t rb64 = (uint64_t)(r0 & ~(TILE - 1)) + (uint64_t)tile * TILE;   // the tile's first receiver, absolute
    if (rb64 >= r1) return;
    const uint32_t rb = (uint32_t)rb64;
    const uint32_t b_diag = rb / BLOCK, b_end = (s1 - 1) / BLOCK + 1;
    const uint64_t lo64 = (uint64_t)(tri ? b_diag : s0 / BLOCK) + (uint64_t)blockIdx.y * SPAN_BLOCKS;
    if (lo64 >= b_end) return;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)min((uint64_t)b_end, lo64 + SPAN_BLOCKS);

    for (uint32_t t = tid; t < W * SLOTS; t += THREADS) (&hist[0][0])[t] = 0;
    if (tid < NB_PAIRS_TABLE) tab[tid] = p.tab[tid];
    __syncthreads();

    const float2 *pos = p.pos + (size_t)member * p.stride;
    float px[K], py[K];
    uint32_t ri[K];
    bool live[K];
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        const uint64_t i = rb64 + k * WAVE + lane;
        live[k] = i >= r0 && i < r1;
        const float2 v = pos[i < r0 ? r0 : i < r1 ? (uint32_t)i : r1 - 1];   // idle lanes redo a receiver of the class; they count nothing
        px[k] = v.x;
        py[k] = v.y;
        ri[k] = (uint32_t)i;
    }

    Counters c;
    c.hist = hist[wid];
    c.tab = tab;
    c.top = p.top;
    c.lane = lane;
    c.c_first = p.c_first;
    c.c_last = p.c_last;
    c.n_first = c.n_last = 0;
    const uint32_t per_wave = (hi - lo + W - 1) / W;
    const uint32_t w_lo = min(lo + wid * per_wave, hi), w_hi = min(w_lo + per_wave, hi);
    const ConstF sp = (ConstF)(uintptr_t)pos;
    for (uint32_t b = w_lo; b < w_hi; b++) {
        const uint32_t j0 = max(b * BLOCK, s0), j1 = (uint32_t)min((uint64_t)(b + 1) * BLOCK, (uint64_t)s1);
        if (tri && b == b_diag)
            block_pairs<true>(c, px, py, ri, live, sp, j0, j1);
        else
            block_pairs<false>(c, px, py, ri, live, sp, j0, j1);
    }
    if (lane == 0) {
        atomicAdd(c.hist + 0, c.n_first);
        atomicAdd(c.hist + p.bins + 1, c.n_last);
    }
    __syncthreads();

    const uint32_t rows = p.bins + 2;
    if (tid <= rows) {
        const uint32_t from = tid < rows ? tid : UNPLACED;
        unsigned long long sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) sum += hist[w][from];
        if (sum) atomicAdd(p.out + ((size_t)member * (rows + 1) + tid) * NB_PAIRS_COLUMNS + cls, sum);
    }
}

}  // namespace
}  // namespace paircount
}  // namespace nb

namespace {

using namespace nbi;
namespace pc = nb::paircount;

// what both calls check of their arguments, before anything touches a device
void check_pairs(const char *what, const float *edges, uint32_t bins, uint32_t classes, const uint64_t *out) {
    NB_ASSERT(edges != nullptr && out != nullptr, "%s: NULL argument", what);
    const char *fault = nb_pair_fault(edges, bins, classes);
    NB_ASSERT(fault == nullptr, "%s: %s (bins %u, classes %u)", what, fault, bins, classes);
}

// the launch over `count` members whose largest has n particles; p holds the members
void launch_pairs(pc::Params &p, const float *edges, uint32_t bins, uint32_t classes, uint32_t count, uint32_t n, hipStream_t stream) {
    p.classes = classes;
    p.bins = bins;
    p.top = nb_pair_thresholds(edges, bins, p.tab);
    p.c_first = p.tab[0];
    p.c_last = p.tab[bins];
    p.tiles = n / pc::TILE + 2;                                           // a class's receivers may start inside a tile
    const uint32_t spans = (n / pc::BLOCK + pc::SPAN_BLOCKS) / pc::SPAN_BLOCKS;   // n / BLOCK + 1 blocks at most
    NB_ASSERT((uint64_t)count * 3 * p.tiles < (1ull << 31), "%u members of %u particles are too many tiles for one launch", count, n);
    ASSERT_HIP(hipMemsetAsync(p.out, 0, (size_t)count * (bins + 3) * NB_PAIRS_COLUMNS * sizeof(uint64_t), stream), "zero the pair counts");
    hipLaunchKernelGGL(pc::pair_count_kernel, dim3(count * 3 * p.tiles, spans), dim3(pc::THREADS), 0, stream, p);
    ASSERT_HIP(hipGetLastError(), "pair_count_kernel launch (%u members of %u, %u bins, classes %u)", count, n, bins, classes);
}

// device layout [rows + 1][3] -> out[rows][3] and unplaced[3]
void unpack(const uint64_t *host, uint32_t rows, uint64_t *out, uint64_t *unplaced) {
    memcpy(out, host, (size_t)rows * NB_PAIRS_COLUMNS * sizeof(uint64_t));
    if (unplaced) memcpy(unplaced, host + (size_t)rows * NB_PAIRS_COLUMNS, NB_PAIRS_COLUMNS * sizeof(uint64_t));
}

uint64_t requested_pairs(uint32_t classes, uint32_t n, uint32_t m) {
    uint64_t pairs = 0;
    for (uint32_t col = 0; col < NB_PAIRS_COLUMNS; col++)
        if ((classes >> col) & 1u) pairs += nb_pair_total(col, n, m);
    return pairs;
}

}  // namespace

extern "C" {

void nb_hip_pair_counts(SimPipeline *s, const float *edges, uint32_t bins, uint32_t classes, uint64_t *out, uint64_t *unplaced) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    check_pairs("nb_hip_pair_counts", edges, bins, classes, out);
    check_diag(s, "nb_hip_pair_counts");
    const uint32_t rows = bins + 2, n = s->data.total_len, m = s->data.mass_len;
    const size_t cells = (size_t)(rows + 1) * NB_PAIRS_COLUMNS;
    if (requested_pairs(classes, n, m) == 0) {
        memset(out, 0, (size_t)rows * NB_PAIRS_COLUMNS * sizeof(uint64_t));
        if (unplaced) memset(unplaced, 0, NB_PAIRS_COLUMNS * sizeof(uint64_t));
        s->read.iv.clear();
        return;
    }
    // the uint64 table the launch adds to: [rows + 1][3]
    const size_t bytes = cells * sizeof(uint64_t);
    const void *host = read_call(s, s->read.iv, "nb_hip_pair_counts", nullptr, 0, bytes, nullptr, bytes, [&](void *, void *work) -> const void * {
        pc::Params p{};
        p.pos = s->pos[s->cur];
        p.n = n;
        p.m = m;
        p.out = static_cast<unsigned long long *>(work);
        launch_pairs(p, edges, bins, classes, 1, n, s->stream);
        return work;
    });
    unpack(static_cast<const uint64_t *>(host), rows, out, unplaced);
}

void nb_hip_ensemble_pair_counts(SimBatch *s, const float *edges, uint32_t bins, uint32_t classes, uint64_t *out, uint64_t *unplaced) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    check_pairs("nb_hip_ensemble_pair_counts", edges, bins, classes, out);
    NB_ASSERT(s->has_data, "nb_hip_ensemble_pair_counts before nb_hip_batch_set_data");
    const uint32_t rows = bins + 2, count = s->count;
    const size_t cells = (size_t)(rows + 1) * NB_PAIRS_COLUMNS;
    uint64_t pairs = 0;
    for (uint32_t b = 0; b < count; b++) pairs += requested_pairs(classes, s->n_len[b], s->mass_len[b]);
    if (pairs == 0) {
        memset(out, 0, (size_t)count * rows * NB_PAIRS_COLUMNS * sizeof(uint64_t));
        if (unplaced) memset(unplaced, 0, (size_t)count * NB_PAIRS_COLUMNS * sizeof(uint64_t));
        s->read.iv.clear();
        return;
    }
    // [count][rows + 1][3] uint64: every member's rows, then its unplaced pairs
    const size_t bytes = count * cells * sizeof(uint64_t);
    const void *landed = read_call(s, s->read.iv, "nb_hip_ensemble_pair_counts", nullptr, 0, bytes, nullptr, bytes, [&](void *, void *work) -> const void * {
        pc::Params p{};
        p.pos = s->pos[s->cur];
        p.mass_len = s->mass_len_dev;
        p.n_len = s->n_len_dev;   // null in a uniform ensemble
        p.n = s->n;
        p.stride = s->stride;
        p.out = static_cast<unsigned long long *>(work);
        launch_pairs(p, edges, bins, classes, count, s->n, s->stream);
        return work;
    });
    const uint64_t *host = static_cast<const uint64_t *>(landed);
    for (uint32_t b = 0; b < count; b++)
        unpack(host + b * cells, rows, out + (size_t)b * rows * NB_PAIRS_COLUMNS, unplaced ? unplaced + (size_t)b * NB_PAIRS_COLUMNS : nullptr);
}

// tuning hook (nbody_hip_tuning.h): the device's threshold table for these edges, NB_PAIRS_TABLE floats; returns top.  Host only.
uint32_t nb_hip_pair_thresholds(const float *edges, uint32_t bins, float *table) {
    check_pairs("nb_hip_pair_thresholds", edges, bins, NB_PAIRS_ALL, reinterpret_cast<const uint64_t *>(table));
    return nb_pair_thresholds(edges, bins, table);
}

}  // extern "C"
