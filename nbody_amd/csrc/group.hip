// group.hip -- the friends-of-friends groups of the state a pipeline or an ensemble holds (include/nbody_group.h): nb_hip_groups
// and nb_hip_ensemble_groups of include/nbody_hip.h.
//
// The statement (which pairs link, the union-find and the argument for it under any interleaving and any stale read) is
// group_common.h, shared with the host path; the range of the mask is neighbour_common.h's, q of a pair and the threshold are
// paircount_common.h's.  A label is the smallest index of a connected component, a property of the link graph alone, so there is
// no order to keep: the result is a function of the state and the arguments.  There is no float atomic; while pairs are merged
// every access to the table is an agent-scope relaxed integer atomic on a global address (load, compare-and-swap, minimum).
//
// Three launches per call, in the stream, for a pipeline (count = 1) and for all members of an ensemble, uniform or ragged; the
// table is [entries] words at the head of the call's scratch, member b's at offsets[b], its values indices within the member:
//   group_init_kernel      parent[i] = i, every call (the scratch holds whatever the last read-only call left)
//   group_pairs_kernel     a workgroup of W = 8 waves owns one tile of 64 * K = 128 receivers of one member and one span of source
//                          blocks, as neighbour.hip's does:
//     half the pairs  a link is symmetric, so only sources j < i are examined: the blocks of 256 up to and including the tile's
//                     own (diagonal) block, the j < i mask in that block only, and none of its sources behind the tile's end
//     sources         every wave walks its own slice of 256 / W = 32 sources of each block of the span; wave-uniform sources
//                     arrive through the scalar cache, 8 per s_load_dwordx16 (loads only), single ones up to the first multiple
//                     of 8 and after the last.  Only particles of the mask are ever addressed
//     pair            v_sub, v_sub, v_mul, v_mul, v_add (the TU builds with -ffp-contract=off: no fma forms q; the K = 2 receivers
//                     of a lane share packed instructions).  A fetch of 8 sources whose least q (v_min3, NaN dropped) is not below
//                     the threshold for any lane of the wave ends there, at one compare per receiver: the common case costs no
//                     memory access.  Otherwise one compare per pair, q < c
//     link            a fetch with a link reads parent[j] of its sources once for the wave, with vector atomic loads (j is
//                     wave-uniform, but the table never goes through the scalar path), all in flight together; each lane keeps
//                     in registers the last root it saw for each of its receivers, and only a lane whose kept root differs from
//                     parent[j] finds root(j) from there, unites the two where they still differ and keeps the root that returns.
//                     Where everything is linked every lane soon holds j's root and parent[j] is that root: a fetch then costs one
//                     round of loads per wave, not N^2 hooks.  A speed device only: dropping it changes no bit
//   group_flatten_kernel   a launch of its own behind the pair launch: group[i] = find(i) for a particle of the mask, NB_GROUP_NONE
//                          for any other, in place -- a label is itself a valid entry of the table (it is of i's tree and <= i)
// No LDS is used.
//
// The span length is a launch parameter and the result is the same for every value of it.  The host's policy (auto_span below)
// counts the triangle: tile t of a member has t / 2 + 1 source blocks, so a launch has about tiles * (blocks + 1) / 2 (tile, block)
// units; the span is that number over two resident rounds of workgroups -- a round is four workgroups of eight waves per CU --
// at least one block, at most all and at most 256 (the tail of the triangle, at auto_span).  A high tile is cut into more spans than a low one; the grid is tiles x the spans of the
// highest tile, and a workgroup whose span starts behind its tile's diagonal block ends at once.  tools/group_probe.py sweeps
// forced lengths beside auto.  nb_hip_group_span (nbody_hip_tuning.h) forces a length, for the tests and that sweep.
//
// Registers: group_pairs_kernel at most 64 VGPRs (64 as built): eight waves per SIMD, so four workgroups of eight waves per CU;
// group_init_kernel and group_flatten_kernel at most 32 (4 and 10 as built).  tests/test_group_cpu.py holds the build to the numbers
// stated here.  No scratch, no LDS.
#include <algorithm>

#include "batch_internal.h"
#include "group_common.h"

namespace nb {
namespace groups {
namespace {

constexpr uint32_t WAVE = 64, K = 2, TILE = WAVE * K, W = 8, THREADS = WAVE * W, BLOCK = 256, SLICE = BLOCK / W, FLAT = 256;
static_assert(BLOCK % TILE == 0 && SLICE % 8 == 0, "a tile lies in one block; a slice is whole fetches");

typedef float v16f __attribute__((ext_vector_type(16)));
typedef const float __attribute__((address_space(4))) *ConstF;   // read-only for the whole launch: scalar loads (positions only)

struct Params {
    const float2 *pos;            // the latest positions; member b's rows start at b * stride
    const uint32_t *mass_len;     // [count] of an ensemble, else null: m
    const uint32_t *n_len;        // [count] of a ragged ensemble, else null: n
    const uint64_t *offsets;      // [count] of a ragged ensemble, else null: member b's entries start at b * n
    uint32_t n, m, stride;
    uint32_t members;             // the mask
    uint32_t tiles;               // grid.x slots per member: of TILE receivers (pairs), of FLAT entries (init, flatten)
    uint32_t span_blocks;         // source blocks per workgroup; grid.y spans
    float c;                      // nb_pair_threshold(linking_length)
    uint32_t *parent;             // [entries]: the table, and in the end the labels
};

// what every kernel derives of its member: counts, the mask's range [lo, hi), the member's table
struct Member {
    uint32_t n, m, lo, hi;
    uint32_t *parent;
};
__device__ __forceinline__ Member member_of(const Params &p, uint32_t member) {
    Member v;
    // the same for every lane, and said so: a loaded value would otherwise count as divergent and take the sources off the scalar cache
    v.n = __builtin_amdgcn_readfirstlane(p.n_len ? p.n_len[member] : p.n);
    v.m = __builtin_amdgcn_readfirstlane(p.mass_len ? p.mass_len[member] : p.m);
    nb_neigh_range(p.members, v.n, v.m, &v.lo, &v.hi);
    v.parent = p.parent + (p.offsets ? p.offsets[member] : (uint64_t)member * p.n);
    return v;
}

__global__ __launch_bounds__(FLAT) void group_init_kernel(const Params p) {
    const uint32_t member = blockIdx.x / p.tiles, i = (blockIdx.x % p.tiles) * FLAT + threadIdx.x;
    const Member v = member_of(p, member);
    if (i < v.n) v.parent[i] = i;
}

__global__ __launch_bounds__(FLAT) void group_flatten_kernel(const Params p) {
    const uint32_t member = blockIdx.x / p.tiles, i = (blockIdx.x % p.tiles) * FLAT + threadIdx.x;
    const Member v = member_of(p, member);
    if (i >= v.n) return;
    const uint32_t label = i >= v.lo && i < v.hi ? nb_group_find(v.parent, i) : NB_GROUP_NONE;
    v.parent[i] = label;
}

// S wave-uniform sources j .. j + S - 1 against the lane's K receivers; MASK: only j < i links (the diagonal block)
template <bool MASK, uint32_t S>
__device__ __forceinline__ void fetch(uint32_t (&root)[K], const float (&px)[K], const float (&py)[K], const uint32_t (&ri)[K],
                                      float c, const float (&sx)[S], const float (&sy)[S], uint32_t j, uint32_t *parent) {
    float q[S][K], least[K];
#pragma unroll
    for (uint32_t u = 0; u < S; u++) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            q[u][k] = nb_pair_q(px[k], py[k], sx[u], sy[u]);
            if (MASK) q[u][k] = j + u < ri[k] ? q[u][k] : __uint_as_float(0x7fc00000u);   // a NaN q links nothing
            least[k] = u ? fminf(least[k], q[u][k]) : q[u][k];   // the smallest that is not NaN
        }
    }
    // Nearly every fetch of a sparse world ends here, at one v_min3 per two pairs and one compare per receiver, with no memory
    // access: where the least q of the fetch is not below the threshold for any lane of the wave, no pair of it links.
    bool any = false;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) any = any || least[k] < c;
    if (__ballot(any) == 0) return;
    uint32_t hits = 0;   // bit u * K + k: source j + u links to receiver k
#pragma unroll
    for (uint32_t u = 0; u < S; u++) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) hits |= (uint32_t)(q[u][k] < c) << (u * K + k);
    }
    // The wave reads parent[j] of the fetch's sources once, together: every lane the same addresses, S loads in flight.  A value of
    // parent[j] is of j's tree for ever; where it is the root a lane keeps for its receiver the two share a tree already and the
    // lane is done with that source at the cost of this one load.  Else the find goes on from that value and the trees are united.
    uint32_t pj[S];
#pragma unroll
    for (uint32_t u = 0; u < S; u++) pj[u] = NB_GROUP_LOAD(parent + (j + u));
#pragma unroll
    for (uint32_t u = 0; u < S; u++) {
        bool apart = false;
#pragma unroll
        for (uint32_t k = 0; k < K; k++) apart = apart || (((hits >> (u * K + k)) & 1u) && root[k] != pj[u]);
        if (!apart) continue;
        const uint32_t rj = nb_group_find(parent, pj[u]);
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            // root[k] is of receiver k's tree and rj of the source's: equal means one tree already; else unite the two trees
            if (((hits >> (u * K + k)) & 1u) && root[k] != rj) root[k] = nb_group_unite(parent, root[k], rj);
        }
    }
}

// the sources [j0, j1) of one slice
template <bool MASK>
__device__ __forceinline__ void slice_pairs(uint32_t (&root)[K], const float (&px)[K], const float (&py)[K], const uint32_t (&ri)[K],
                                            float c, ConstF sp, uint32_t j0, uint32_t j1, uint32_t *parent) {
    auto one = [&](uint32_t j) {
        const float sx[1] = {sp[2 * (size_t)j]}, sy[1] = {sp[2 * (size_t)j + 1]};
        fetch<MASK, 1>(root, px, py, ri, c, sx, sy, j, parent);
    };
    uint32_t j = j0;
    for (; j < j1 && (j & 7u); j++) one(j);
    for (; j + 8 <= j1; j += 8) {
        const v16f P = *(const v16f __attribute__((address_space(4))) *)(sp + 2 * (size_t)j);
        float sx[8], sy[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) sx[u] = P[2 * u], sy[u] = P[2 * u + 1];
        fetch<MASK, 8>(root, px, py, ri, c, sx, sy, j, parent);
    }
    for (; j < j1; j++) one(j);
}

__global__ __launch_bounds__(THREADS) void group_pairs_kernel(const Params p) {
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const uint32_t member = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const Member v = member_of(p, member);
    const uint32_t r0 = v.lo, r1 = v.hi;   // receivers and sources: the mask's range
    if (r1 <= r0 + 1) return;
    const uint64_t rb64 = (uint64_t)(r0 & ~(TILE - 1)) + (uint64_t)tile * TILE;   // the tile's first receiver, absolute
    if (rb64 >= r1) return;
    const uint32_t rb = (uint32_t)rb64;
    const uint32_t b_diag = rb / BLOCK;
    const uint64_t lo64 = (uint64_t)(r0 / BLOCK) + (uint64_t)blockIdx.y * p.span_blocks;
    if (lo64 > b_diag) return;   // the triangle: no block behind the tile's own
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)min((uint64_t)b_diag + 1, lo64 + p.span_blocks);
    const uint32_t s1 = (uint32_t)min((uint64_t)r1, rb64 + TILE);   // no receiver of the tile lies behind this, so no source j < i does

    const float2 *pos = p.pos + (size_t)member * p.stride;
    float px[K], py[K];
    uint32_t ri[K], root[K];
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        const uint64_t i = rb64 + k * WAVE + lane;
        const bool live = i >= r0 && i < r1;
        const float2 w = pos[i < r0 ? r0 : i < r1 ? (uint32_t)i : r1 - 1];   // idle lanes address a receiver of the mask ...
        px[k] = live ? w.x : __uint_as_float(0x7fc00000u);                   // ... and stand at NaN: every q of theirs is NaN and links nothing
        py[k] = w.y;
        ri[k] = (uint32_t)i;
        root[k] = live ? (uint32_t)i : r0;   // a particle is of its own tree
    }

    const ConstF sp = (ConstF)(uintptr_t)pos;
    for (uint32_t b = lo; b < hi; b++) {
        const uint64_t first = (uint64_t)b * BLOCK + wid * SLICE;
        const uint32_t j0 = (uint32_t)max(first, (uint64_t)r0), j1 = (uint32_t)min(first + SLICE, (uint64_t)s1);
        if (first >= s1 || j0 >= j1) continue;
        if (b == b_diag)
            slice_pairs<true>(root, px, py, ri, p.c, sp, j0, j1, v.parent);
        else
            slice_pairs<false>(root, px, py, ri, p.c, sp, j0, j1, v.parent);
    }
}

}  // namespace
}  // namespace groups
}  // namespace nb

namespace {

using namespace nbi;
namespace gr = nb::groups;

std::atomic<uint32_t> g_forced_span{0};   // nb_hip_group_span: 0 = auto

// what both calls check of their arguments, before anything touches a device
void check_groups(const char *what, uint32_t members, float linking_length, const uint32_t *group) {
    NB_ASSERT(group != nullptr, "%s: NULL argument", what);
    const char *fault = nb_group_fault(members, linking_length);
    NB_ASSERT(fault == nullptr, "%s: %s (members %u, linking_length %g)", what, fault, members, (double)linking_length);
}

// The policy of the span length, in blocks of 256 sources: a launch over `count` members of `tiles` tiles and `blocks` source
// blocks each examines the triangle j < i, about count * tiles * (blocks + 1) / 2 (tile, block) units.  The span is that over
// two resident rounds of the chip (a round: four workgroups of eight waves per CU): one block while the units do not reach two
// rounds; and at most 256 blocks however many units there are, because the highest tile has `blocks` of them and the lowest one:
// uncut, the launch ends on the workgroups of its highest tiles (N = 2^20, 4 097 blocks: spans of 64 to 256 blocks take 8 %
// less than one span, profiles/r29_group_probe.json).  Any value gives the same result.
uint32_t auto_span(uint64_t count, uint32_t tiles, uint32_t blocks, int compute_units) {
    const uint64_t want = 2ull * 4ull * (uint64_t)(compute_units > 0 ? compute_units : 1);
    const uint64_t units = count * tiles * ((uint64_t)blocks + 1) / 2;
    const uint64_t longest = std::max<uint64_t>(256, ((uint64_t)blocks + 65534) / 65535);   // a launch holds 65 535 spans
    const uint64_t span = std::min({units / want, (uint64_t)blocks, longest});
    return (uint32_t)(span < 1 ? 1 : span);
}

// the three launches over `count` members whose largest has n particles; p holds the members and the table
void launch_groups(gr::Params &p, uint32_t members, float linking_length, uint32_t count, uint32_t n, hipStream_t stream) {
    p.members = members;
    p.c = nb_pair_threshold(linking_length);
    const uint32_t flat_tiles = n / gr::FLAT + 1, pair_tiles = n / gr::TILE + 1;
    NB_ASSERT((uint64_t)count * pair_tiles < (1ull << 31), "%u members of %u particles are too many tiles for one launch", count, n);
    const uint32_t blocks = n / gr::BLOCK + 1, forced = g_forced_span.load();
    p.span_blocks = forced ? forced : auto_span(count, pair_tiles, blocks, g_dev.compute_units);
    const uint32_t spans = (blocks + p.span_blocks - 1) / p.span_blocks;
    NB_ASSERT(spans <= 65535u, "a span of %u blocks cuts %u particles into %u spans: more than one launch holds", p.span_blocks, n, spans);

    p.tiles = flat_tiles;
    hipLaunchKernelGGL(gr::group_init_kernel, dim3(count * flat_tiles), dim3(gr::FLAT), 0, stream, p);
    ASSERT_HIP(hipGetLastError(), "group_init_kernel launch (%u members of %u)", count, n);
    p.tiles = pair_tiles;
    hipLaunchKernelGGL(gr::group_pairs_kernel, dim3(count * pair_tiles, spans), dim3(gr::THREADS), 0, stream, p);
    ASSERT_HIP(hipGetLastError(), "group_pairs_kernel launch (%u members of %u, span %u blocks, members %u)", count, n, p.span_blocks, members);
    p.tiles = flat_tiles;
    hipLaunchKernelGGL(gr::group_flatten_kernel, dim3(count * flat_tiles), dim3(gr::FLAT), 0, stream, p);
    ASSERT_HIP(hipGetLastError(), "group_flatten_kernel launch (%u members of %u)", count, n);
}

// can a world of n particles, m of them massive, hold a link under this mask and length
bool anything(uint32_t members, float linking_length, uint32_t n, uint32_t m) {
    uint32_t lo, hi;
    nb_neigh_range(members, n, m, &lo, &hi);
    return linking_length > 0.0f && hi > lo + 1;
}

}  // namespace

extern "C" {

void nb_hip_groups(SimPipeline *s, uint32_t members, float linking_length, uint32_t *group, uint32_t *n_groups) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    check_groups("nb_hip_groups", members, linking_length, group);
    check_diag(s, "nb_hip_groups");
    const uint32_t n = s->data.total_len, m = s->data.mass_len;
    if (!anything(members, linking_length, n, m)) {
        nb_group_defaults(n, m, members, group);
        s->read.iv.clear();
    } else {
        const size_t bytes = (size_t)n * sizeof(uint32_t);
        read_call(s, s->read.iv, "nb_hip_groups", nullptr, 0, bytes, group, bytes, [&](void *, void *work) -> const void * {
            gr::Params p{};
            p.pos = s->pos[s->cur];
            p.n = n;
            p.m = m;
            p.parent = static_cast<uint32_t *>(work);
            launch_groups(p, members, linking_length, 1, n, s->stream);
            return work;
        });
    }
    if (n_groups) *n_groups = nb_group_count(group, n);
}

void nb_hip_ensemble_groups(SimBatch *s, uint32_t members, float linking_length, uint32_t *group, uint32_t *n_groups) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    check_groups("nb_hip_ensemble_groups", members, linking_length, group);
    NB_ASSERT(s->has_data, "nb_hip_ensemble_groups before nb_hip_batch_set_data");
    const uint64_t entries = s->offsets[s->count];
    bool any = false;
    for (uint32_t b = 0; b < s->count; b++) any = any || anything(members, linking_length, s->n_len[b], s->mass_len[b]);
    if (!any) {
        for (uint32_t b = 0; b < s->count; b++) nb_group_defaults(s->n_len[b], s->mass_len[b], members, group + s->offsets[b]);
        s->read.iv.clear();
    } else {
        const size_t bytes = (size_t)entries * sizeof(uint32_t);
        read_call(s, s->read.iv, "nb_hip_ensemble_groups", nullptr, 0, bytes, group, bytes, [&](void *, void *work) -> const void * {
            gr::Params p{};
            p.pos = s->pos[s->cur];
            p.mass_len = s->mass_len_dev;
            p.n_len = s->n_len_dev;       // null in a uniform ensemble, like the offsets
            p.offsets = s->offsets_dev;
            p.n = s->n;
            p.stride = s->stride;
            p.parent = static_cast<uint32_t *>(work);
            launch_groups(p, members, linking_length, s->count, s->n, s->stream);
            return work;
        });
    }
    if (n_groups)
        for (uint32_t b = 0; b < s->count; b++) n_groups[b] = nb_group_count(group + s->offsets[b], s->n_len[b]);
}

// tuning hook (nbody_hip_tuning.h): source blocks per workgroup of the next calls, process-wide; 0 = auto.  Returns the previous value.
uint32_t nb_hip_group_span(uint32_t blocks) { return g_forced_span.exchange(blocks); }

}  // extern "C"
