// convert.hip -- the utility kernels around the force path: AoS <-> SoA split / merge, inert pads, G*m, fills, for one
// world and for whole ensembles.  None of them is on the hot path of a step; each rule they share (the record layout,
// the G*m rounding, the inert pad) is written once below.
#include "convert.h"

namespace nb {
namespace {

struct alignas(16) ParticleRec {  // == Particle (include/nbody.h): pos vel | acc mass radius
    float4 a, b;
};

struct Soa {  // one particle as the SoA arrays hold it
    float2 pos, vel, acc;
    float mass, radius;
};

__device__ __forceinline__ Soa unpack(const ParticleRec &r) {
    return {make_float2(r.a.x, r.a.y), make_float2(r.a.z, r.a.w), make_float2(r.b.x, r.b.y), r.b.z, r.b.w};
}

__device__ __forceinline__ ParticleRec pack(const Soa &s) {
    return {make_float4(s.pos.x, s.pos.y, s.vel.x, s.vel.y), make_float4(s.acc.x, s.acc.y, s.mass, s.radius)};
}

// the inert pad: far away, finite, massless: contributes exactly 0 as a source and stays finite as a receiver
__device__ __forceinline__ Soa inert_pad() {
    return {make_float2(1.0e15f, 1.0e15f), make_float2(0.f, 0.f), make_float2(0.f, 0.f), 0.0f, 1.0f};
}

// G*m of a source.  `g` is the host's NB_G (include/nbody.h), handed in at launch like the reference's specialisation
// constant (sim_gpu.c:54-72, particle_cs.glsl:26): the device code holds no copy of the value.
__device__ __forceinline__ float g_times_m(float m, float g) {
    return m > 0.0f ? __fmul_rn(m, g) : 0.0f;  // rounded as the reference's `gm = m * g` (sim_cpu.c:179)
}

__device__ __forceinline__ void store_soa(const Soa &s, size_t o, float2 *pos, float2 *vel, float2 *acc, float *radius, float *mass) {
    pos[o] = s.pos;
    vel[o] = s.vel;
    acc[o] = s.acc;
    mass[o] = s.mass;
    radius[o] = s.radius;
}

__device__ __forceinline__ Soa load_soa(size_t o, const float2 *pos, const float2 *vel, const float2 *acc, const float *radius,
                                        const float *mass) {
    return {pos[o], vel[o], acc[o], mass[o], radius[o]};
}

__global__ void split_kernel(const ParticleRec *aos, uint32_t first, uint32_t count, float2 *pos, float2 *vel, float2 *acc,
                             float *radius, float *mass, uint32_t slot0) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    store_soa(unpack(aos[first + i]), slot0 + i, pos, vel, acc, radius, mass);
}

__global__ void merge_kernel(ParticleRec *aos, uint32_t first, uint32_t count, const float2 *pos, const float2 *vel,
                             const float2 *acc, const float *radius, const float *mass, uint32_t slot0) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    aos[first + i] = pack(load_soa(slot0 + i, pos, vel, acc, radius, mass));
}

__global__ void fill_pad_kernel(float2 *pos, float2 *vel, float2 *acc, float *radius, float *mass, uint32_t slot0,
                                uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    store_soa(inert_pad(), slot0 + i, pos, vel, acc, radius, mass);
}

// dst[0 .. count) = value; the step-size upload is the one-thread launch of it
__global__ void fill_kernel(float *dst, uint32_t count, float value) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = value;
}

__global__ void make_gm_kernel(const float *mass, float *gm, uint32_t count, float g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    gm[i] = g_times_m(mass[i], g);
}

// Sharded upload: the gathered source arrays (both ping-pong buffers) and the static G*m straight from the AoS
// world every rank holds.  Slots past mass_len are inert pads.
__global__ void split_sources_kernel(const ParticleRec *aos, uint32_t mass_len, uint32_t n_src, float2 *pos0, float2 *pos1,
                                     float *gm, float g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_src) return;
    const Soa s = i < mass_len ? unpack(aos[i]) : inert_pad();
    pos0[i] = s.pos;
    pos1[i] = s.pos;
    gm[i] = g_times_m(s.mass, g);
}

// Where member b's AoS records are and how many it has: all that the converters of a uniform and of a ragged ensemble
// differ in (the step kernels' member_of, kernels.hip, mirrored).  Each converter is one template over the two.
struct UniformRecords {   // every member has n records, member b's at b * n
    uint32_t n;
};

struct RaggedRecords {    // member b has n_len[b] records, packed at offsets[b]; both arrays on the device
    const uint64_t *offsets;
    const uint32_t *n_len;
};

struct Records {
    uint32_t n;
    size_t first;
};

__device__ __forceinline__ Records records_of(const UniformRecords &u, uint32_t b) { return {u.n, (size_t)b * u.n}; }
__device__ __forceinline__ Records records_of(const RaggedRecords &r, uint32_t b) { return {r.n_len[b], r.offsets[b]}; }

// Ensemble upload: member blockIdx.y's AoS records into its SoA rows, and G*m of its sources (rows past mass_len[b]
// hold no source and get 0).  One launch for the whole ensemble.
template <class A>
__global__ void batch_split_kernel(const ParticleRec *aos, const uint32_t *mass_len, const A where, uint32_t stride, float2 *pos,
                                   float2 *vel, float2 *acc, float *radius, float *mass, float *gm, float g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const Records rec = records_of(where, b);
    if (i >= rec.n) return;
    const Soa s = unpack(aos[rec.first + i]);
    const size_t o = (size_t)b * stride + i;
    store_soa(s, o, pos, vel, acc, radius, mass);
    gm[o] = i < mass_len[b] ? g_times_m(s.mass, g) : 0.0f;
}

// Ensemble read-back: members [first, first + gridDim.y) back into their AoS records.
template <class A>
__global__ void batch_merge_kernel(ParticleRec *aos, uint32_t first, const A where, uint32_t stride, const float2 *pos,
                                   const float2 *vel, const float2 *acc, const float *radius, const float *mass) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, b = first + blockIdx.y;
    const Records rec = records_of(where, b);
    if (i >= rec.n) return;
    aos[rec.first + i] = pack(load_soa((size_t)b * stride + i, pos, vel, acc, radius, mass));
}

// The position rows of the listed members from one ping-pong buffer to the other (ragged ensembles: the chain group's
// members step in place while the lane-split groups flip buffers).
__global__ void ragged_copy_rows_kernel(const uint32_t *members, const uint32_t *n_len, uint32_t stride, const float2 *from, float2 *to) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, b = members[blockIdx.y];
    if (i >= n_len[b]) return;
    const size_t o = (size_t)b * stride + i;
    to[o] = from[o];
}

inline dim3 grid1d(uint32_t count, uint32_t rows = 1) { return dim3((count + 255u) / 256u, rows); }

}  // namespace

void launch_ragged_copy_rows(hipStream_t st, const uint32_t *members, const uint32_t *n_len, uint32_t count, uint32_t max_n,
                             uint32_t stride, const float2 *from, float2 *to) {
    if (count) hipLaunchKernelGGL(ragged_copy_rows_kernel, grid1d(max_n, count), dim3(256), 0, st, members, n_len, stride, from, to);
}

void launch_batch_split(hipStream_t st, const void *aos, const uint64_t *offsets, const uint32_t *n_len, const uint32_t *mass_len,
                        uint32_t count, uint32_t n, uint32_t stride, float2 *pos, float2 *vel, float2 *acc, float *radius, float *mass,
                        float *gm, float g) {
    const ParticleRec *recs = static_cast<const ParticleRec *>(aos);
    const UniformRecords uniform = {n};
    const RaggedRecords ragged = {offsets, n_len};
    if (n_len)
        hipLaunchKernelGGL(batch_split_kernel<RaggedRecords>, grid1d(n, count), dim3(256), 0, st, recs, mass_len, ragged, stride, pos, vel,
                           acc, radius, mass, gm, g);
    else
        hipLaunchKernelGGL(batch_split_kernel<UniformRecords>, grid1d(n, count), dim3(256), 0, st, recs, mass_len, uniform, stride, pos,
                           vel, acc, radius, mass, gm, g);
}

void launch_batch_merge(hipStream_t st, void *aos, const uint64_t *offsets, const uint32_t *n_len, uint32_t first, uint32_t count,
                        uint32_t n, uint32_t stride, const float2 *pos, const float2 *vel, const float2 *acc, const float *radius,
                        const float *mass) {
    if (count == 0) return;
    ParticleRec *recs = static_cast<ParticleRec *>(aos);
    const UniformRecords uniform = {n};
    const RaggedRecords ragged = {offsets, n_len};
    if (n_len)
        hipLaunchKernelGGL(batch_merge_kernel<RaggedRecords>, grid1d(n, count), dim3(256), 0, st, recs, first, ragged, stride, pos, vel, acc,
                           radius, mass);
    else
        hipLaunchKernelGGL(batch_merge_kernel<UniformRecords>, grid1d(n, count), dim3(256), 0, st, recs, first, uniform, stride, pos, vel,
                           acc, radius, mass);
}

void launch_batch_fill(hipStream_t st, float *dst, uint32_t count, float value) {
    hipLaunchKernelGGL(fill_kernel, grid1d(count), dim3(256), 0, st, dst, count, value);
}

void launch_set_scalar(hipStream_t st, float *dst, float value) {
    hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(1), 0, st, dst, 1u, value);
}

void launch_split(hipStream_t st, const void *aos, uint32_t first, uint32_t count, float2 *pos, float2 *vel, float2 *acc,
                  float *radius, float *mass, uint32_t slot0) {
    if (count) hipLaunchKernelGGL(split_kernel, grid1d(count), dim3(256), 0, st, static_cast<const ParticleRec *>(aos), first, count,
                       pos, vel, acc, radius, mass, slot0);
}

void launch_fill_pad(hipStream_t st, float2 *pos, float2 *vel, float2 *acc, float *radius, float *mass, uint32_t slot0,
                     uint32_t count) {
    if (count) hipLaunchKernelGGL(fill_pad_kernel, grid1d(count), dim3(256), 0, st, pos, vel, acc, radius, mass, slot0, count);
}

void launch_make_gm(hipStream_t st, const float *mass, float *gm, uint32_t count, float g) {
    if (count) hipLaunchKernelGGL(make_gm_kernel, grid1d(count), dim3(256), 0, st, mass, gm, count, g);
}

void launch_merge(hipStream_t st, void *aos, uint32_t first, uint32_t count, const float2 *pos, const float2 *vel,
                  const float2 *acc, const float *radius, const float *mass, uint32_t slot0) {
    if (count) hipLaunchKernelGGL(merge_kernel, grid1d(count), dim3(256), 0, st, static_cast<ParticleRec *>(aos), first, count, pos,
                       vel, acc, radius, mass, slot0);
}

void launch_split_sources(hipStream_t st, const void *aos, uint32_t mass_len, uint32_t n_src, float2 *pos0, float2 *pos1,
                          float *gm, float g) {
    if (n_src) hipLaunchKernelGGL(split_sources_kernel, grid1d(n_src), dim3(256), 0, st, static_cast<const ParticleRec *>(aos), mass_len,
                       n_src, pos0, pos1, gm, g);
}

}  // namespace nb
