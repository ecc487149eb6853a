// neighbour.hip -- the nearest neighbour and the neighbour count of every particle of the state a pipeline or an ensemble holds
// (include/nbody_neighbour.h): nb_hip_neighbours and nb_hip_ensemble_neighbours of include/nbody_hip.h.
//
// The statement (the ranges of the masks, what a pair does to a receiver, the key) is neighbour_common.h, shared with the host
// path; q of a pair and the count's threshold are paircount_common.h's.  The result is a minimum over 64-bit keys and an integer
// count, so there is no order to keep: partial results meet through integer atomics and the result is still a function of the
// state and the arguments alone.  There is no float atomic; every store to global memory is one of the two integer atomics.
//
// neighbour_kernel<COUNT>, one launch for a pipeline (count = 1) and for all members of an ensemble, uniform or ragged; two
// instances, nearest only and nearest + count.  A workgroup of W = 8 waves owns one tile of 64 * K = 128 receivers of one member
// and one span of source blocks:
//   tiles     and source blocks of 256 are cut in ABSOLUTE index, so a tile lies inside one block, and only that (diagonal) block
//             takes the j != i mask: there a pair with the receiver's own index gets a NaN q, which is never a candidate
//   sources   every wave walks its own slice of 256 / W = 32 sources of each block of the span, so all waves work whatever the
//             span's length; wave-uniform sources arrive through the scalar cache, 8 per s_load_dwordx16 (loads only), single
//             ones up to the first multiple of 8 and after the last.  Only sources of the source mask and receivers of the
//             receiver mask are ever addressed
//   pair      v_sub, v_sub, v_mul, v_mul, v_add (the TU builds with -ffp-contract=off: no fma forms q; the K = 2 receivers of a
//             lane share packed instructions), then one compare and two selects (q, j); with COUNT one more compare against the
//             threshold and an integer add.  A wave meets its sources in increasing j and takes a strictly smaller q only: the
//             smallest index among equal q.  The compare and the selects of a fetch of 8 sources run only when the least of its
//             q (v_min3, NaN dropped) lies below what some lane of the wave holds; otherwise no pair of the fetch would be taken
//   close     every lane turns its (q, j) into a key and the W waves meet in LDS: one ds_min_u64 and, with COUNT, one ds_add_u32
//             per receiver and wave.  Then thread t issues one 64-bit atomicMin (a single global_atomic_umin_x2, no
//             compare-and-swap loop) and one 32-bit atomicAdd for receiver t of the tile into the call's table; a receiver
//             without a candidate in this span, or with a count of zero, issues none.  The host sets the keys to all ones and the
//             counts to zero in the stream before the launch, and decodes a key whose low word is NB_NEIGH_NONE to (+inf, NONE)
//
// The span length is a launch parameter and the result is the same for every value of it.  The host's policy (auto_span below):
// as many spans as bring the launch to two resident rounds of workgroups -- a round is four workgroups of eight waves per CU --
// and no more than there are blocks.  A small world has too few tiles to fill the chip (N = 6 000 is 47 tiles for 256 CUs: 24
// spans of one block), and a launch of half a round ends on its slowest CU (N = 65 536 in one span is 513 workgroups: two on most
// CUs, three on some).  More spans than that cost: every span starts from "nothing held", so the early end of a fetch (above)
// fires less often.  tools/neighbour_probe.py sweeps forced lengths beside auto (profiles/r28_neighbour_probe.json).
// nb_hip_neighbour_span (nbody_hip_tuning.h) forces a length, for the tests and that sweep.
//
// Registers: neighbour_kernel<false> at most 64 VGPRs (45 as built), neighbour_kernel<true> at most 64 (62 as built): eight waves
// per SIMD, so four workgroups of eight waves per CU (tests/test_neighbour_cpu.py holds the build to the numbers stated here), no
// scratch.  LDS: 128 x 8 B of keys + 128 x 4 B of counts = 1.5 KiB per workgroup (the nearest-only instance: the keys, 1.0 KiB).
#include "batch_internal.h"
#include "neighbour_common.h"

namespace nb {
namespace neighbour {
namespace {

constexpr uint32_t WAVE = 64, K = 2, TILE = WAVE * K, W = 8, THREADS = WAVE * W, BLOCK = 256, SLICE = BLOCK / W;
static_assert(BLOCK % TILE == 0 && SLICE % 8 == 0 && TILE <= THREADS, "a tile lies in one block; a slice is whole fetches; one thread per receiver");

typedef float v16f __attribute__((ext_vector_type(16)));
typedef const float __attribute__((address_space(4))) *ConstF;   // read-only for the whole launch: scalar loads

struct Params {
    const float2 *pos;            // the latest positions; member b's rows start at b * stride
    const uint32_t *mass_len;     // [count] of an ensemble, else null: m
    const uint32_t *n_len;        // [count] of a ragged ensemble, else null: n
    const uint64_t *offsets;      // [count] of a ragged ensemble, else null: member b's entries start at b * n
    uint32_t n, m, stride;
    uint32_t receivers, sources;  // the masks
    uint32_t tiles;               // grid.x slots per member
    uint32_t span_blocks;         // source blocks per workgroup; grid.y spans
    float c;                      // nb_pair_threshold(radius)
    unsigned long long *keys;     // [entries], all ones
    uint32_t *counts;             // [entries], zeroed; COUNT only
};

struct Best {
    float q[K];
    uint32_t j[K], within[K];
};

// S wave-uniform sources j .. j + S - 1 against the lane's K receivers; MASK: the receiver's own index is no candidate (the diagonal block)
template <bool MASK, bool COUNT, uint32_t S>
__device__ __forceinline__ void group(Best &b, const float (&px)[K], const float (&py)[K], const uint32_t (&ri)[K], float c, const float (&sx)[S],
                                      const float (&sy)[S], uint32_t j) {
    float q[S][K], least[K];
#pragma unroll
    for (uint32_t u = 0; u < S; u++) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            q[u][k] = nb_pair_q(px[k], py[k], sx[u], sy[u]);
            if (MASK) q[u][k] = j + u == ri[k] ? __uint_as_float(0x7fc00000u) : q[u][k];
            if (COUNT) b.within[k] += q[u][k] < c;
            least[k] = u ? fminf(least[k], q[u][k]) : q[u][k];   // the smallest that is not NaN
        }
    }
    // A pair is taken only when its q lies below what the receiver holds, and what it holds only falls: where the least q of the
    // group is not below it for any lane of the wave, nothing would be taken and the group ends here.  A receiver's held q falls
    // about ln(sources) times, so nearly every group of a long walk ends here, at one v_min3 per two pairs instead of a compare
    // and two selects per pair; the groups that do not are offered pair by pair, in increasing j, as the statement says.
    bool closer = false;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) closer = closer || least[k] < b.q[k];
    if (__ballot(closer) == 0) return;
#pragma unroll
    for (uint32_t u = 0; u < S; u++) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) nb_neigh_take(q[u][k], j + u, &b.q[k], &b.j[k]);
    }
}

// the sources [j0, j1) of one slice
template <bool MASK, bool COUNT>
__device__ __forceinline__ void slice_pairs(Best &b, const float (&px)[K], const float (&py)[K], const uint32_t (&ri)[K], float c, ConstF sp,
                                            uint32_t j0, uint32_t j1) {
    auto one = [&](uint32_t j) {
        const float sx[1] = {sp[2 * (size_t)j]}, sy[1] = {sp[2 * (size_t)j + 1]};
        group<MASK, COUNT, 1>(b, px, py, ri, c, sx, sy, j);
    };
    uint32_t j = j0;
    for (; j < j1 && (j & 7u); j++) one(j);
    for (; j + 8 <= j1; j += 8) {
        const v16f P = *(const v16f __attribute__((address_space(4))) *)(sp + 2 * (size_t)j);
        float sx[8], sy[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) sx[u] = P[2 * u], sy[u] = P[2 * u + 1];
        group<MASK, COUNT, 8>(b, px, py, ri, c, sx, sy, j);
    }
    for (; j < j1; j++) one(j);
}

template <bool COUNT>
__global__ __launch_bounds__(THREADS) void neighbour_kernel(const Params p) {
    __shared__ unsigned long long skey[TILE];
    __shared__ uint32_t swithin[TILE];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const uint32_t member = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    // the same for every lane, and said so: a loaded value would otherwise count as divergent and take the sources off the scalar cache
    const uint32_t n = __builtin_amdgcn_readfirstlane(p.n_len ? p.n_len[member] : p.n);
    const uint32_t m = __builtin_amdgcn_readfirstlane(p.mass_len ? p.mass_len[member] : p.m);
    uint32_t r0, r1, s0, s1;   // receivers [r0, r1), sources [s0, s1)
    nb_neigh_range(p.receivers, n, m, &r0, &r1);
    nb_neigh_range(p.sources, n, m, &s0, &s1);
    if (r1 <= r0 || s1 <= s0) return;
    const uint64_t rb64 = (uint64_t)(r0 & ~(TILE - 1)) + (uint64_t)tile * TILE;   // the tile's first receiver, absolute
    if (rb64 >= r1) return;
    const uint32_t rb = (uint32_t)rb64;
    const uint32_t b_diag = rb / BLOCK, b_end = (s1 - 1) / BLOCK + 1;
    const uint64_t lo64 = (uint64_t)(s0 / BLOCK) + (uint64_t)blockIdx.y * p.span_blocks;
    if (lo64 >= b_end) return;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)min((uint64_t)b_end, lo64 + p.span_blocks);

    if (tid < TILE) {
        skey[tid] = NB_NEIGH_KEY_NONE;
        swithin[tid] = 0;
    }
    __syncthreads();

    const float2 *pos = p.pos + (size_t)member * p.stride;
    float px[K], py[K];
    uint32_t ri[K];
    bool live[K];
    Best best;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        const uint64_t i = rb64 + k * WAVE + lane;
        live[k] = i >= r0 && i < r1;
        const float2 v = pos[i < r0 ? r0 : i < r1 ? (uint32_t)i : r1 - 1];   // idle lanes redo a receiver of the mask; they report nothing
        px[k] = v.x;
        py[k] = v.y;
        ri[k] = (uint32_t)i;
        best.q[k] = __uint_as_float(0x7f800000u);
        best.j[k] = NB_NEIGH_NONE;
        best.within[k] = 0;
    }

    const ConstF sp = (ConstF)(uintptr_t)pos;
    for (uint32_t b = lo; b < hi; b++) {
        const uint64_t first = (uint64_t)b * BLOCK + wid * SLICE;
        const uint32_t j0 = (uint32_t)max(first, (uint64_t)s0), j1 = (uint32_t)min(first + SLICE, (uint64_t)s1);
        if (first >= s1 || j0 >= j1) continue;
        if (b == b_diag)
            slice_pairs<true, COUNT>(best, px, py, ri, p.c, sp, j0, j1);
        else
            slice_pairs<false, COUNT>(best, px, py, ri, p.c, sp, j0, j1);
    }

#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        if (!live[k]) continue;
        const unsigned long long key = nb_neigh_key(best.q[k], best.j[k]);
        if (key != NB_NEIGH_KEY_NONE) atomicMin(&skey[k * WAVE + lane], key);
        if (COUNT && best.within[k]) atomicAdd(&swithin[k * WAVE + lane], best.within[k]);
    }
    __syncthreads();

    const uint64_t i = rb64 + tid;
    if (tid < TILE && i >= r0 && i < r1) {
        const uint64_t at = (p.offsets ? p.offsets[member] : (uint64_t)member * p.n) + i;
        const unsigned long long key = skey[tid];
        if (key != NB_NEIGH_KEY_NONE) atomicMin(p.keys + at, key);
        if (COUNT) {
            const uint32_t within = swithin[tid];
            if (within) atomicAdd(p.counts + at, within);
        }
    }
}

}  // namespace
}  // namespace neighbour
}  // namespace nb

namespace {

using namespace nbi;
namespace ng = nb::neighbour;

std::atomic<uint32_t> g_forced_span{0};   // nb_hip_neighbour_span: 0 = auto

// what both calls check of their arguments, before anything touches a device
void check_neighbours(const char *what, uint32_t receivers, uint32_t sources, float radius, const float *q, const uint32_t *index, const uint32_t *count) {
    NB_ASSERT(q != nullptr && index != nullptr, "%s: NULL argument", what);
    const char *fault = nb_neigh_fault(receivers, sources, radius, count != nullptr);
    NB_ASSERT(fault == nullptr, "%s: %s (receivers %u, sources %u, radius %g)", what, fault, receivers, sources, (double)radius);
}

// The policy of the span length, in blocks of 256 sources: the launch has `tiles` (member, tile) slots, a member at most `blocks`
// source blocks.  Spans multiply the workgroups; as many as reach two resident rounds of the chip (a round: four workgroups of
// eight waves per CU), never more than there are blocks, and one span once the tiles alone reach it.  Any value gives the same
// result.
uint32_t auto_span(uint64_t tiles, uint32_t blocks, int compute_units) {
    const uint64_t want = 2ull * 4ull * (uint64_t)(compute_units > 0 ? compute_units : 1);
    uint64_t spans = (want + (tiles ? tiles : 1) - 1) / (tiles ? tiles : 1);
    spans = spans > blocks ? blocks : spans;
    return (uint32_t)((blocks + spans - 1) / spans);
}

// the launch over `count` members whose largest has n particles and that hold `entries` particles together; p holds the members
void launch_neighbours(ng::Params &p, uint32_t receivers, uint32_t sources, float radius, bool counted, uint32_t count, uint32_t n, uint64_t entries,
                       void *work, hipStream_t stream) {
    p.receivers = receivers;
    p.sources = sources;
    p.c = counted ? nb_pair_threshold(radius) : 0.0f;
    p.tiles = n / ng::TILE + 1;
    NB_ASSERT((uint64_t)count * p.tiles < (1ull << 31), "%u members of %u particles are too many tiles for one launch", count, n);
    const uint32_t blocks = n / ng::BLOCK + 1, forced = g_forced_span.load();
    p.span_blocks = forced ? forced : auto_span((uint64_t)count * p.tiles, blocks, g_dev.compute_units);
    const uint32_t spans = (blocks + p.span_blocks - 1) / p.span_blocks;
    NB_ASSERT(spans <= 65535u, "a span of %u blocks cuts %u particles into %u spans: more than one launch holds", p.span_blocks, n, spans);
    // the table: [entries] keys, then [entries] counts
    p.keys = static_cast<unsigned long long *>(work);
    p.counts = reinterpret_cast<uint32_t *>(p.keys + entries);
    ASSERT_HIP(hipMemsetAsync(p.keys, 0xff, entries * sizeof(uint64_t), stream), "set the neighbour keys");
    if (counted) ASSERT_HIP(hipMemsetAsync(p.counts, 0, entries * sizeof(uint32_t), stream), "zero the neighbour counts");
    const dim3 grid(count * p.tiles, spans), block(ng::THREADS);
    if (counted)
        hipLaunchKernelGGL(ng::neighbour_kernel<true>, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(ng::neighbour_kernel<false>, grid, block, 0, stream, p);
    ASSERT_HIP(hipGetLastError(), "neighbour_kernel launch (%u members of %u, span %u blocks, receivers %u, sources %u)", count, n, p.span_blocks,
               receivers, sources);
}

// does a world of n particles, m of them massive, have a receiver and a source under these masks
bool anything(uint32_t receivers, uint32_t sources, uint32_t n, uint32_t m) {
    uint32_t r0, r1, s0, s1;
    nb_neigh_range(receivers, n, m, &r0, &r1);
    nb_neigh_range(sources, n, m, &s0, &s1);
    return r1 > r0 && s1 > s0;
}

// the copied-back table -> the caller's arrays
void unpack(const void *host, uint64_t entries, float *q, uint32_t *index, uint32_t *count) {
    const uint64_t *keys = static_cast<const uint64_t *>(host);
    for (uint64_t i = 0; i < entries; i++) nb_neigh_decode(keys[i], &q[i], &index[i]);
    if (count) memcpy(count, keys + entries, entries * sizeof(uint32_t));
}

}  // namespace

extern "C" {

void nb_hip_neighbours(SimPipeline *s, uint32_t receivers, uint32_t sources, float radius, float *q, uint32_t *index, uint32_t *count) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    check_neighbours("nb_hip_neighbours", receivers, sources, radius, q, index, count);
    check_diag(s, "nb_hip_neighbours");
    const uint32_t n = s->data.total_len, m = s->data.mass_len;
    if (!anything(receivers, sources, n, m)) {
        nb_neigh_defaults(n, q, index, count);
        s->read.iv.clear();
        return;
    }
    const size_t bytes = (size_t)n * (count ? 12 : 8);
    const void *host = read_call(s, s->read.iv, "nb_hip_neighbours", nullptr, 0, (size_t)n * 12, nullptr, bytes, [&](void *, void *work) -> const void * {
        ng::Params p{};
        p.pos = s->pos[s->cur];
        p.n = n;
        p.m = m;
        launch_neighbours(p, receivers, sources, radius, count != nullptr, 1, n, n, work, s->stream);
        return work;
    });
    unpack(host, n, q, index, count);
}

void nb_hip_ensemble_neighbours(SimBatch *s, uint32_t receivers, uint32_t sources, float radius, float *q, uint32_t *index, uint32_t *count) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    check_neighbours("nb_hip_ensemble_neighbours", receivers, sources, radius, q, index, count);
    NB_ASSERT(s->has_data, "nb_hip_ensemble_neighbours before nb_hip_batch_set_data");
    const uint64_t entries = s->offsets[s->count];
    bool any = false;
    for (uint32_t b = 0; b < s->count; b++) any = any || anything(receivers, sources, s->n_len[b], s->mass_len[b]);
    if (!any) {
        nb_neigh_defaults(entries, q, index, count);
        s->read.iv.clear();
        return;
    }
    const size_t bytes = (size_t)entries * (count ? 12 : 8);
    const void *host = read_call(s, s->read.iv, "nb_hip_ensemble_neighbours", nullptr, 0, (size_t)entries * 12, nullptr, bytes, [&](void *, void *work) -> const void * {
        ng::Params p{};
        p.pos = s->pos[s->cur];
        p.mass_len = s->mass_len_dev;
        p.n_len = s->n_len_dev;       // null in a uniform ensemble, like the offsets
        p.offsets = s->offsets_dev;
        p.n = s->n;
        p.stride = s->stride;
        launch_neighbours(p, receivers, sources, radius, count != nullptr, s->count, s->n, entries, work, s->stream);
        return work;
    });
    unpack(host, entries, q, index, count);
}

// tuning hook (nbody_hip_tuning.h): source blocks per workgroup of the next calls, process-wide; 0 = auto.  Returns the previous value.
uint32_t nb_hip_neighbour_span(uint32_t blocks) { return g_forced_span.exchange(blocks); }

}  // extern "C"
