// render_kernels.hip -- the render kernels of a world (a SimPipeline: render.hip) and of an ensemble (a SimBatch:
// batch_observe.hip) and their launchers (render_kernels.h).  What the two share is written once: the constants, the disc
// list's item (Disc), the bounds reduction (reduce_keys) and the disc append (append_disc).
//
// Definitions: include/nbody_render.h; the per-particle and per-pixel arithmetic is render_common.h, the same inline
// functions the host path (render_cpu.c) compiles.  Every result is an integer sum or an integer min / max, so the order in
// which lanes, waves and workgroups arrive cannot change a bit: no float atomics anywhere, and member b's image is bit for
// bit the image of the same particles rendered alone.  An ensemble's SoA is read as batch.hip lays it out: member b's rows
// start at b * stride and only rows [0, n) exist (the pad rows hold zeros: walking them would put phantom particles at the
// origin).
//
// reduce_keys              x and y of the finite particles as ordered unsigned keys (-0 below +0), min / max per lane, across
//                          the wave by shuffles, across the workgroup's waves through LDS.  bounds_kernel walks a world in
//                          a grid stride and ends in four no-return global_atomic_umin / umax per workgroup;
//                          ensemble_bounds_kernel gives a member one workgroup, which owns keys[b]: four plain stores, no
//                          atomics, no identity memset.
// splat_kernel             a world.  One lane = PER_LANE particles of pos[cur] / mass / radius (all loads issued before the
//                          first add).  A particle is classified and becomes nothing, a point or a disc.  Discs whose
//                          candidate box meets the image are appended to a compact list (append_disc).  Points are added to
//                          the count image.  Zoomed out, half a million particles land in a handful of words, so lanes that
//                          hit the same word are merged first: the first live lane's word is broadcast (v_readlane), the
//                          lanes that match it are counted (ballot + popcount) and leave, and their sum waits in a
//                          wave-uniform pending (word, count) pair per class that the next item of the same wave can add to;
//                          a pair is written with ONE no-return global_atomic_add_u32 when its word changes or the wave
//                          ends.  A round that merges fewer than MERGE_MIN lanes means the words are spread: the lanes still
//                          live then add 1 each in one vector atomic and the item is done, so a spread view pays one
//                          broadcast and one compare per item.
// ensemble_splat_kernel    an ensemble's global path (tiles above TILE_LDS_BYTES), members along blockIdx.y, one lane = one
//                          particle, classified with member b's own view, one atomic per point; the discs of all members
//                          go to ONE list whose items carry the member.
// disc_kernel              a disc's work is its clipped candidate box.  It is cut into DISC_SLICES interleaved row sets, one
//                          wave each, lanes along x: a core zoomed to fill 1280 x 720 runs on 64 waves, a 7-pixel star on 7.
//                          Waves walk (disc, slice) items in a grid stride; the disc count is read from device memory, so
//                          the host never waits for the splat.  ensemble_disc_kernel is the same walk with the member's
//                          planes found from the item; shared, it cost a world 3 - 4 % of a disc-heavy 4096 x 4096 view
//                          (profiles/r21_render_kernels.json), so a world keeps the kernel without the member arithmetic.
// shade_kernel             one pixel per lane: the integer formula of the header, one packed RGBA word stored.
//                          ensemble_shade_kernel walks members * plane pixels and divides to find the member; shared, the
//                          division cost a world 3 - 6 % of its shade (same profile), so a world keeps its own.
// ensemble_tile_kernel     an ensemble's tile path (3 * width * height * 4 bytes <= TILE_LDS_BYTES): one workgroup per member
//                          keeps the member's whole tile in LDS.  Zero it, walk the member's particles in passes of TILE_PASS
//                          (classified with member b's own view): points add 1 with a no-return LDS atomic, discs that can
//                          touch the tile go, with their clipped candidate box, to an LDS list that one pass cannot
//                          overflow; after a barrier the waves walk the list -- a wave per disc while its box is small, the
//                          whole workgroup per disc above that -- with LDS atomics.  After the last barrier the tile leaves
//                          with plain coalesced stores; the <true> build shades each pixel straight from LDS instead and
//                          stores only the frame.  No clear, no global atomics, no disc list in HBM, one launch.
#include "render_kernels.h"

#include "render_common.h"

namespace nb {
namespace render {

constexpr uint32_t WAVE = 64;
constexpr uint32_t THREADS = 256;
constexpr uint32_t WAVES = THREADS / WAVE;
constexpr int PER_LANE = 8;                   // splat: particles per lane
constexpr uint32_t MERGE_MIN = 4;             // splat: a round that merges fewer lanes ends the merging of its item
constexpr uint32_t DISC_SLICES = 64;          // waves a disc's rows are dealt to
constexpr uint32_t DISC_GROUPS = 1024;
constexpr uint32_t BOUNDS_GROUPS_MAX = 256;   // one workgroup per compute unit, a grid stride beyond
constexpr uint32_t NO_WORD = 0xffffffffu;     // no count-image word: the image has at most 3 * 2^24 of them
constexpr uint32_t TILE_PASS = 512;           // particles per pass of the tile kernel = items of its LDS disc list (12 KiB)
constexpr uint32_t SMALL_BOX = 256;           // tile kernel: candidate pixels up to which one wave takes a disc alone

struct ViewParams {
    float tx, ty, ox, oy, zoom, core_mass;
    uint32_t width, height;
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d /= 2) v = min(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d /= 2) v = max(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
    return v;
}

// The ordered keys of pos[first], pos[first + step], ... below n, reduced over the workgroup: thread t < 4 returns the min key
// of x, of y, the max key of x, of y (the identities when no particle is finite); the other threads return nothing of use.
__device__ __forceinline__ uint32_t reduce_keys(const float2 *pos, uint32_t n, uint32_t first, uint32_t step) {
    uint32_t lo_x = NB_RENDER_KEY_NONE_MIN, lo_y = NB_RENDER_KEY_NONE_MIN;
    uint32_t hi_x = NB_RENDER_KEY_NONE_MAX, hi_y = NB_RENDER_KEY_NONE_MAX;
    for (uint32_t i = first; i < n; i += step) {
        const float2 p = pos[i];
        // & and not &&: one condition for the four selects below (with && the ensemble's loop compiles to 8 more v_cndmask)
        if (!(nb_render_finite(p.x) & nb_render_finite(p.y))) continue;
        const uint32_t kx = nb_render_order_key(p.x), ky = nb_render_order_key(p.y);
        lo_x = min(lo_x, kx);
        hi_x = max(hi_x, kx);
        lo_y = min(lo_y, ky);
        hi_y = max(hi_y, ky);
    }
    lo_x = wave_min(lo_x);
    lo_y = wave_min(lo_y);
    hi_x = wave_max(hi_x);
    hi_y = wave_max(hi_y);
    __shared__ uint32_t part[WAVES][4];
    const uint32_t wid = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        part[wid][0] = lo_x;
        part[wid][1] = lo_y;
        part[wid][2] = hi_x;
        part[wid][3] = hi_y;
    }
    __syncthreads();
    uint32_t v = 0;
    if (threadIdx.x < 4) {
        v = part[0][threadIdx.x];
#pragma unroll
        for (uint32_t w = 1; w < WAVES; w++) v = threadIdx.x < 2 ? min(v, part[w][threadIdx.x]) : max(v, part[w][threadIdx.x]);
    }
    return v;
}

// the four waves meet in LDS first: four adds on ONE cache line per workgroup (the line takes ~88 atomics per microsecond)
__global__ __launch_bounds__(THREADS) void bounds_kernel(const float2 *pos, uint32_t n, uint32_t *keys) {
    const uint32_t v = reduce_keys(pos, n, blockIdx.x * THREADS + threadIdx.x, gridDim.x * THREADS);
    if (threadIdx.x < 4) {
        if (threadIdx.x < 2)
            atomicMin(&keys[threadIdx.x], v);
        else
            atomicMax(&keys[threadIdx.x], v);
    }
}

__global__ __launch_bounds__(THREADS) void ensemble_bounds_kernel(const float2 *pos, uint32_t n, uint32_t stride, uint32_t *keys) {
    const uint32_t v = reduce_keys(pos + (size_t)blockIdx.x * stride, n, threadIdx.x, THREADS);
    if (threadIdx.x < 4) keys[(size_t)blockIdx.x * 4 + threadIdx.x] = v;
}

// The lanes of a wave that hold a disc append it to a list in device memory: ONE returning add per wave, by the first of
// them (ballot + popcount); each then stores behind the lanes below it.
__device__ __forceinline__ void append_disc(bool disc, const Disc &item, uint32_t lane, Disc *discs, uint32_t *ndisc) {
    const uint64_t dmask = __ballot(disc);
    if (dmask == 0) return;
    const int first = __ffsll((unsigned long long)dmask) - 1;
    uint32_t at = 0;
    if ((int)lane == first) at = atomicAdd(ndisc, (uint32_t)__popcll(dmask));
    at = (uint32_t)__builtin_amdgcn_readlane((int)at, first);
    if (disc) discs[at + (uint32_t)__popcll(dmask & ((1ull << lane) - 1ull))] = item;
}

// a wave-uniform pending (word, count): flushed by one lane with one no-return add
struct Pending {
    uint32_t word = NO_WORD, count = 0;
};

__device__ __forceinline__ void flush(Pending &p, uint32_t *counts, uint32_t lane) {
    if (p.count != 0 && lane == 0) atomicAdd(&counts[p.word], p.count);
    p.word = NO_WORD;
    p.count = 0;
}

__device__ __forceinline__ void pend(Pending &p, uint32_t word, uint32_t count, uint32_t *counts, uint32_t lane) {
    if (p.word != word) {
        flush(p, counts, lane);
        p.word = word;
    }
    p.count += count;
}

template <bool MERGE>
__global__ __launch_bounds__(THREADS) void splat_kernel(const float2 *pos, const float *mass, const float *radius, uint32_t n,
                                                        const ViewParams v, uint32_t *counts, Disc *discs, uint32_t *ndisc) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = (blockIdx.x * THREADS + threadIdx.x) / WAVE;
    const uint32_t base = wave * (WAVE * PER_LANE);
    const uint32_t plane = v.width * v.height;

    float2 p[PER_LANE];
    float m[PER_LANE], r[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
        const uint32_t i = base + k * WAVE + lane;
        const uint32_t c = i < n ? i : n - 1;   // tail lanes reload the last particle; it is not counted twice (live below)
        p[k] = pos[c];
        m[k] = mass[c];
        r[k] = radius[c];
    }

    Pending pending[NB_RENDER_CLASSES];
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
        const bool live = base + k * WAVE + lane < n;
        NbSplat s;
        const int kind = nb_render_classify(p[k].x, p[k].y, m[k], r[k], v.tx, v.ty, v.ox, v.oy, v.zoom, v.core_mass, &s);

        // discs that can touch the image
        uint32_t x0, x1, y0, y1;
        const bool disc = live && kind == NB_RENDER_DISC && nb_render_disc_span(s.sx, s.rho, v.width, &x0, &x1) &&
                          nb_render_disc_span(s.sy, s.rho, v.height, &y0, &y1);
        append_disc(disc, Disc{s.sx, s.sy, s.rho, s.cls}, lane, discs, ndisc);

        // points in view
        uint32_t px = 0, py = 0;
        const bool point = live && kind == NB_RENDER_POINT && nb_render_point_pixel(s.sx, s.sy, v.width, v.height, &px, &py);
        const uint32_t word = s.cls * plane + py * v.width + px;
        if constexpr (!MERGE) {
            if (point) atomicAdd(&counts[word], 1u);
        } else {
            uint64_t act = __ballot(point);
            while (act != 0) {
                const int first = __ffsll((unsigned long long)act) - 1;
                const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)word, first);
                const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)s.cls, first);
                const uint64_t same = __ballot(point && word == w0) & act;
                const uint32_t cnt = (uint32_t)__popcll(same);
                if (cnt < MERGE_MIN) {   // spread words: what is left adds 1 per lane, in one vector atomic
                    if ((act >> lane) & 1ull) atomicAdd(&counts[word], 1u);
                    break;
                }
                act &= ~same;
                if (c0 == 0)
                    pend(pending[0], w0, cnt, counts, lane);
                else if (c0 == 1)
                    pend(pending[1], w0, cnt, counts, lane);
                else
                    pend(pending[2], w0, cnt, counts, lane);
            }
        }
    }
    if constexpr (MERGE) {
#pragma unroll
        for (int c = 0; c < NB_RENDER_CLASSES; c++) flush(pending[c], counts, lane);
    }
}

// one lane = one particle of member blockIdx.y; counts[count][3][plane], *ndisc cleared with them
__global__ __launch_bounds__(THREADS) void ensemble_splat_kernel(const EnsembleRenderParams p, uint32_t *counts, Disc *discs,
                                                                 uint32_t *ndisc) {
    const uint32_t b = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    const uint32_t plane = p.width * p.height;
    const bool live = i < p.n;   // rows [n, stride) are padding
    const RenderView v = p.views[b];
    const size_t row = (size_t)b * p.stride + (live ? i : 0u);
    const float2 xy = p.pos[row];
    NbSplat s;
    const int kind = nb_render_classify(xy.x, xy.y, p.mass[row], p.radius[row], v.target[0], v.target[1], v.offset[0], v.offset[1], v.zoom,
                                        v.core_mass, &s);
    uint32_t x0, x1, y0, y1;
    const bool disc = live && kind == NB_RENDER_DISC && nb_render_disc_span(s.sx, s.rho, p.width, &x0, &x1) &&
                      nb_render_disc_span(s.sy, s.rho, p.height, &y0, &y1);
    append_disc(disc, Disc{s.sx, s.sy, s.rho, s.cls | (b << 2)}, lane, discs, ndisc);
    uint32_t px = 0, py = 0;
    if (live && kind == NB_RENDER_POINT && nb_render_point_pixel(s.sx, s.sy, p.width, p.height, &px, &py))
        atomicAdd(&counts[((size_t)b * NB_RENDER_CLASSES + s.cls) * plane + py * p.width + px], 1u);
}

__global__ __launch_bounds__(THREADS) void disc_kernel(const Disc *discs, const uint32_t *ndisc, uint32_t width, uint32_t height,
                                                       uint32_t *counts) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * THREADS + threadIdx.x) / WAVE);
    const uint32_t waves = gridDim.x * WAVES;
    const uint64_t items = (uint64_t)*ndisc * DISC_SLICES;
    const uint32_t plane = width * height;
    for (uint64_t it = wave; it < items; it += waves) {
        const Disc s = discs[it / DISC_SLICES];
        const uint32_t slice = (uint32_t)(it % DISC_SLICES);
        uint32_t x0, x1, y0, y1;
        if (!nb_render_disc_span(s.sx, s.rho, width, &x0, &x1) || !nb_render_disc_span(s.sy, s.rho, height, &y0, &y1)) continue;
        uint32_t *img = counts + s.cls_member * plane;   // a world is member 0
        for (uint32_t py = y0 + slice; py <= y1; py += DISC_SLICES)
            for (uint32_t px = x0 + lane; px <= x1; px += WAVE)
                if (nb_render_disc_covers(s.sx, s.sy, s.rho, px, py)) atomicAdd(&img[py * width + px], 1u);
    }
}

// disc_kernel over the one list of an ensemble: counts[count][3][plane]
__global__ __launch_bounds__(THREADS) void ensemble_disc_kernel(const Disc *discs, const uint32_t *ndisc, uint32_t width, uint32_t height,
                                                                uint32_t *counts) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * THREADS + threadIdx.x) / WAVE);
    const uint32_t waves = gridDim.x * WAVES;
    const uint64_t items = (uint64_t)*ndisc * DISC_SLICES;
    const uint32_t plane = width * height;
    for (uint64_t it = wave; it < items; it += waves) {
        const Disc s = discs[it / DISC_SLICES];
        const uint32_t slice = (uint32_t)(it % DISC_SLICES);
        uint32_t x0, x1, y0, y1;
        if (!nb_render_disc_span(s.sx, s.rho, width, &x0, &x1) || !nb_render_disc_span(s.sy, s.rho, height, &y0, &y1)) continue;
        uint32_t *img = counts + ((size_t)(s.cls_member >> 2) * NB_RENDER_CLASSES + (s.cls_member & 3u)) * plane;
        for (uint32_t py = y0 + slice; py <= y1; py += DISC_SLICES)
            for (uint32_t px = x0 + lane; px <= x1; px += WAVE)
                if (nb_render_disc_covers(s.sx, s.sy, s.rho, px, py)) atomicAdd(&img[py * width + px], 1u);
    }
}

__global__ __launch_bounds__(THREADS) void shade_kernel(const uint32_t *counts, uint32_t plane, const RenderPalette pal, uint32_t *rgba) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= plane) return;
    rgba[i] = nb_render_shade_pixel(counts[i], counts[plane + i], counts[2 * plane + i], &pal);
}

// counts[count][3][plane] -> rgba[count][plane]; pixels = count * plane
__global__ __launch_bounds__(THREADS) void ensemble_shade_kernel(const uint32_t *counts, uint32_t plane, uint32_t pixels,
                                                                 const RenderPalette pal, uint32_t *rgba) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= pixels) return;
    const uint32_t b = i / plane;
    const uint32_t *c = counts + (size_t)b * NB_RENDER_CLASSES * plane + (i - b * plane);
    rgba[i] = nb_render_shade_pixel(c[0], c[plane], c[2u * plane], &pal);
}

// ---- the tile path ------------------------------------------------------------------------------------------------------

// the pixels of one disc's clipped candidate box, flattened and dealt to `step` lanes starting at `first`
__device__ __forceinline__ void add_disc(const NbSplat &s, uint32_t x0, uint32_t y0, uint32_t bw, uint32_t area, uint32_t first,
                                         uint32_t step, uint32_t width, uint32_t *img) {
    for (uint32_t i = first; i < area; i += step) {
        const uint32_t py = y0 + i / bw, px = x0 + i % bw;
        if (nb_render_disc_covers(s.sx, s.sy, s.rho, px, py)) atomicAdd(&img[py * width + px], 1u);
    }
}

template <bool SHADE>
__global__ __launch_bounds__(THREADS) void ensemble_tile_kernel(const EnsembleRenderParams p, uint32_t *counts, const RenderPalette pal,
                                                                uint32_t *rgba) {
    extern __shared__ uint32_t tile[];        // [3][height][width]
    __shared__ NbSplat discs[TILE_PASS];      // small boxes from the front, large ones from the back: a pass appends <= TILE_PASS
    __shared__ uint2 boxes[TILE_PASS];        // the clipped candidate box of discs[d]: {x0 | bw << 16, y0 | bh << 16}
    __shared__ uint32_t ndisc[2][2];          // [pass & 1][small, large]: the cursors of the even and of the odd passes
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1), wid = tid / WAVE;
    const uint32_t width = p.width, height = p.height;
    const uint32_t plane = width * height, words = plane * NB_RENDER_CLASSES;

    for (uint32_t i = tid; i < words; i += THREADS) tile[i] = 0u;
    if (tid < 4) ndisc[tid / 2][tid % 2] = 0u;
    const RenderView v = p.views[b];
    const size_t row0 = (size_t)b * p.stride;
    __syncthreads();

    for (uint32_t base = 0, pass = 0; base < p.n; base += TILE_PASS, pass++) {
        uint32_t *cursor = ndisc[pass & 1u];
#pragma unroll
        for (uint32_t k = 0; k < TILE_PASS / THREADS; k++) {
            const uint32_t i = base + k * THREADS + tid;
            if (i >= p.n) continue;   // rows [n, stride) are padding
            const float2 xy = p.pos[row0 + i];
            NbSplat s;
            const int kind = nb_render_classify(xy.x, xy.y, p.mass[row0 + i], p.radius[row0 + i], v.target[0], v.target[1], v.offset[0],
                                                v.offset[1], v.zoom, v.core_mass, &s);
            uint32_t px, py, x0, x1, y0, y1;
            if (kind == NB_RENDER_POINT) {
                if (nb_render_point_pixel(s.sx, s.sy, width, height, &px, &py)) atomicAdd(&tile[s.cls * plane + py * width + px], 1u);
            } else if (kind == NB_RENDER_DISC) {
                if (nb_render_disc_span(s.sx, s.rho, width, &x0, &x1) && nb_render_disc_span(s.sy, s.rho, height, &y0, &y1)) {
                    // the tile has at most TILE_LDS_BYTES / 12 pixels, so every coordinate and extent fits 16 bits
                    const uint32_t bw = x1 - x0 + 1u, bh = y1 - y0 + 1u;
                    const uint32_t d = bw * bh <= SMALL_BOX ? atomicAdd(&cursor[0], 1u) : TILE_PASS - 1u - atomicAdd(&cursor[1], 1u);
                    discs[d] = s;
                    boxes[d] = make_uint2(x0 | bw << 16, y0 | bh << 16);
                }
            }
        }
        __syncthreads();
        const uint32_t nsmall = cursor[0], nlarge = cursor[1];
        if (tid < 2) ndisc[(pass + 1u) & 1u][tid] = 0u;   // last read before this pass's first barrier, next written after its last
        // small boxes: a wave per disc
        for (uint32_t d = wid; d < nsmall; d += WAVES) {
            const NbSplat s = discs[d];
            const uint2 box = boxes[d];
            const uint32_t bw = box.x >> 16;
            add_disc(s, box.x & 0xffffu, box.y & 0xffffu, bw, bw * (box.y >> 16), lane, WAVE, width, tile + s.cls * plane);
        }
        // large boxes: the whole workgroup per disc
        for (uint32_t k = 0; k < nlarge; k++) {
            const uint32_t d = TILE_PASS - 1u - k;
            const NbSplat s = discs[d];
            const uint2 box = boxes[d];
            const uint32_t bw = box.x >> 16;
            add_disc(s, box.x & 0xffffu, box.y & 0xffffu, bw, bw * (box.y >> 16), tid, THREADS, width, tile + s.cls * plane);
        }
        __syncthreads();
    }

    if constexpr (SHADE) {
        uint32_t *out = rgba + (size_t)b * plane;
        for (uint32_t i = tid; i < plane; i += THREADS) out[i] = nb_render_shade_pixel(tile[i], tile[plane + i], tile[2u * plane + i], &pal);
    } else {
        uint32_t *out = counts + (size_t)b * words;
        for (uint32_t i = tid; i < words; i += THREADS) out[i] = tile[i];
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------

void launch_bounds(hipStream_t stream, const float2 *pos, uint32_t n, uint32_t *keys) {
    const uint32_t groups = (n + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(bounds_kernel, dim3(groups < BOUNDS_GROUPS_MAX ? groups : BOUNDS_GROUPS_MAX), dim3(THREADS), 0, stream, pos, n, keys);
}

void launch_splat(hipStream_t stream, const float2 *pos, const float *mass, const float *radius, uint32_t n, const RenderView &view,
                  bool merge, uint32_t *counts, Disc *discs, uint32_t *ndisc) {
    const ViewParams v = {view.target[0], view.target[1], view.offset[0], view.offset[1], view.zoom, view.core_mass, view.width, view.height};
    const uint32_t per_group = THREADS * PER_LANE;
    hipLaunchKernelGGL(merge ? splat_kernel<true> : splat_kernel<false>, dim3((n + per_group - 1) / per_group), dim3(THREADS), 0, stream,
                       pos, mass, radius, n, v, counts, discs, ndisc);
}

void launch_discs(hipStream_t stream, const Disc *discs, const uint32_t *ndisc, uint32_t width, uint32_t height, uint32_t *counts) {
    hipLaunchKernelGGL(disc_kernel, dim3(DISC_GROUPS), dim3(THREADS), 0, stream, discs, ndisc, width, height, counts);
}

void launch_shade(hipStream_t stream, const uint32_t *counts, uint32_t plane, const RenderPalette &palette, uint32_t *rgba) {
    hipLaunchKernelGGL(shade_kernel, dim3((plane + THREADS - 1) / THREADS), dim3(THREADS), 0, stream, counts, plane, palette, rgba);
}

void launch_ensemble_bounds(hipStream_t stream, const float2 *pos, uint32_t n, uint32_t stride, uint32_t count, uint32_t *keys) {
    hipLaunchKernelGGL(ensemble_bounds_kernel, dim3(count), dim3(THREADS), 0, stream, pos, n, stride, keys);
}

void launch_ensemble_tile(hipStream_t stream, const EnsembleRenderParams &p, uint32_t *counts, const RenderPalette *palette,
                          uint32_t *rgba) {
    const size_t lds = (size_t)p.width * p.height * NB_RENDER_CLASSES * sizeof(uint32_t);
    if (palette)
        hipLaunchKernelGGL(ensemble_tile_kernel<true>, dim3(p.count), dim3(THREADS), lds, stream, p, counts, *palette, rgba);
    else
        hipLaunchKernelGGL(ensemble_tile_kernel<false>, dim3(p.count), dim3(THREADS), lds, stream, p, counts, RenderPalette{}, rgba);
}

void launch_ensemble_global(hipStream_t stream, const EnsembleRenderParams &p, uint32_t *counts, Disc *discs) {
    uint32_t *ndisc = counts + (global_count_words(p.count, p.width, p.height) - 1);
    hipLaunchKernelGGL(ensemble_splat_kernel, dim3((p.n + THREADS - 1) / THREADS, p.count), dim3(THREADS), 0, stream, p, counts, discs,
                       ndisc);
    hipLaunchKernelGGL(ensemble_disc_kernel, dim3(DISC_GROUPS), dim3(THREADS), 0, stream, discs, ndisc, p.width, p.height, counts);
}

void launch_ensemble_shade(hipStream_t stream, const uint32_t *counts, uint32_t count, uint32_t plane, const RenderPalette &palette,
                           uint32_t *rgba) {
    const uint32_t pixels = count * plane;
    hipLaunchKernelGGL(ensemble_shade_kernel, dim3((pixels + THREADS - 1) / THREADS), dim3(THREADS), 0, stream, counts, plane, pixels,
                       palette, rgba);
}

}  // namespace render
}  // namespace nb
