// step_tile.inc -- the body of a step launch as TEXT: one workgroup computes receiver tile `tile_x` against source part
// `part_y`.  Included inside every kernel that runs it (kernels.hip: step_kernel, which reads the pair off its block index,
// and dealt_kernel, which draws it from a ticket), with in scope: the template arguments K, W, VARIANT, FUSED, SRC_CONSTANT (src_load), the
// parameter block `const StepParams p` -- the kernel's own by-value argument -- and `const uint32_t tile_x, part_y`.
// Text and not a device function on purpose: with the body in a force-inlined function that takes the parameter block by
// reference (or by value, or reads it off the kernarg segment) the compiler loads the whole block at kernel entry instead
// of field by field where each is used, and all 22 step_kernel instantiations change their scalar register allocation
// (K = 2 then spills SGPRs into VGPR lanes).  As text the step kernels compile to the instruction streams they had
// (profiles/r23_deal_isa.txt).  Part of the kernel-source hash (benchlib.KERNEL_SOURCES).
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1);
    // wave id as an SGPR value so that everything derived from it stays scalar
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);

    // per wave, double-buffered: 64 interleaved (x, y) pairs, then 64 G*m
    __shared__ __attribute__((aligned(16))) float tile[VARIANT == VARIANT_LDS ? W : 1][2][3 * CHUNK];
    __shared__ float2 partial[W > 1 ? W : 1][W > 1 ? WAVE * K : 1];

    // the step size: a scalar load issued first, consumed by the epilogue.  (Fetching the integrating thread's velocity
    // and position here as well, instead of after the force loop, measured 0.1 us per step SLOWER at N = 250 ... 1 000:
    // profiles/r02_ab_early_fetch.txt.)
    const float dt = *p.dt;

    const uint32_t recv_base = tile_x * (WAVE * K);
    Receivers<K> R;
#pragma unroll
    for (int k = 0; k < K; k++) {
        uint32_t i = recv_base + k * WAVE + lane;
        i = i < p.n_recv ? i : p.n_recv - 1;  // tail lanes redo the last receiver; their stores are masked
        i = receiver_slot(p, i);
        const float2 q = p.pos_in[i];
        R.p[k] = f2v{q.x, q.y};
        R.r[k] = p.radius[i];
    }
    R.clear();

    // the concatenated source ranges
    const uint32_t n0 = p.src_end[0] - p.src_begin[0];
    const uint32_t n1 = p.src_end[1] - p.src_begin[1];
    const uint32_t total = n0 + n1;
    // this workgroup's part of the sources (all of them unless the step is split), then this wave's slice of it, both
    // in whole granules of p.unit sources (64 = one tile; finer for latency-bound launches, see StepParams::unit)
    const SourceSlice wave_src = source_slice(total, p.unit, p.split, part_y, W, wid);
    const uint32_t v_lo = wave_src.lo;   // first source of the slice: a multiple of 8
    const uint32_t v_hi = wave_src.hi;   // one past its last source

    if constexpr (VARIANT == VARIANT_LDS) {
        float(*T)[3 * CHUNK] = tile[wid];
        float2 sp = make_float2(0.f, 0.f);
        float sg = 0.f;
        auto fetch = [&](uint32_t c) {
            const uint32_t v = c * CHUNK + lane;
            const bool live = v < total;
            const uint32_t j = source_index(p, live ? v : total - 1, n0);
            sp = p.src_pos[j];                 // 512 B per wave, coalesced
            sg = live ? p.src_gm[j] : 0.0f;    // pad sources: a real position, zero mass
        };
        // whole 64-source tiles only: this route always runs with the 64-source granule (choose_shape), so the slice
        // is [c_lo, c_hi) tiles and the last one may be ragged (pads: a real position, zero mass)
        const uint32_t c_lo = v_lo / CHUNK, c_hi = (v_hi + CHUNK - 1) / CHUNK;
        if (c_lo < c_hi) fetch(c_lo);
        int buf = 0;
        for (uint32_t c = c_lo; c < c_hi; c++) {
            *reinterpret_cast<float2 *>(&T[buf][2 * lane]) = sp;  // ds_write_b64
            T[buf][2 * CHUNK + lane] = sg;
            if (c + 1 < c_hi) fetch(c + 1);  // next tile's HBM/L2 latency hides under this tile's math
            // LDS executes one wave's accesses in order; this only stops the compiler from reordering
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int jj = 0; jj < CHUNK; jj += 4) {
                // broadcast ds_read_b128: every lane reads the same 16 bytes.  Four sources per read group (two reads
                // of positions, one of G*m): 12 staging VGPRs instead of 24, which is what leaves room for the
                // paired-rsq body with two receivers per lane
                const v8f P = *reinterpret_cast<const v8f *>(&T[buf][2 * jj]);
                const v4f G = *reinterpret_cast<const v4f *>(&T[buf][2 * CHUNK + jj]);
#pragma unroll
                for (int u = 0; u < 4; u++) interact<K, false>(R, f2v{P[2 * u], P[2 * u + 1]}, G[u]);
            }
            if (((c - c_lo) & (CLOSE_EVERY - 1)) == CLOSE_EVERY - 1) R.close_chunk();
            buf ^= 1;
        }
        if ((c_hi - c_lo) & (CLOSE_EVERY - 1)) R.close_chunk();  // a short last block
    } else {
        // scalar-cache route: indices are wave-uniform, the loads become s_load_dwordx8/x16
#pragma unroll
        for (int range = 0; range < 2; range++) {
            // intersection of [v_lo, v_hi) with this range, as indices of the source arrays
            const uint32_t r_lo = range == 0 ? 0u : n0;
            const uint32_t r_hi = range == 0 ? n0 : total;
            const uint32_t a = max(v_lo, r_lo), b = min(v_hi, r_hi);
            if (a >= b) continue;
            uint32_t j = p.src_begin[range] + (a - r_lo);
            const uint32_t j_end = p.src_begin[range] + (b - r_lo);
            // 8 sources per scalar fetch: s_load_dwordx16 (x,y pairs) + s_load_dwordx8 (G*m).  Slices start on
            // multiples of 64 sources from 64-aligned range starts, so j is a multiple of 8 here.
            const float *sp = reinterpret_cast<const float *>(p.src_pos), *sg = p.src_gm;
            // every 8 * CLOSE_EVERY groups (256 sources) the block sums are closed, exactly where the LDS variant
            // closes them, so both variants add in the same order; a short last block may end in single sources
            const uint32_t groups = (j_end - j) / 8;
            const uint32_t g0 = (a - v_lo) / 8;  // groups of this slice that lie in the previous range
            if (groups > 0) {
                // Two register sets, A and B, each fetched while the other one is being consumed (the scalar
                // cache's latency hides under 8 * K interactions) and each dead before its refill is issued, so
                // no set is ever copied.  g0 is even (range starts are 64-aligned) and a block ends on an odd
                // group index, so only the second group of a pair can close one.  The refill address is clamped to
                // the last group instead of branching around the load.
                const uint32_t j_last = j + (groups - 1) * 8;
                v16f PA = src_load<v16f, SRC_CONSTANT>(sp + 2 * (size_t)j);
                v8f GA = src_load<v8f, SRC_CONSTANT>(sg + j);
                uint32_t g = 0;
                while (g + 2 <= groups) {
                    // pairs up to the end of the current 32-group block, as one branch-free inner loop
                    const uint32_t to_close = (8u * CLOSE_EVERY - ((g0 + g) & (8u * CLOSE_EVERY - 1))) / 2;
                    const uint32_t pairs = min(to_close, (groups - g) / 2);
                    for (uint32_t i = 0; i < pairs; i++) {
                        // Scalar loads return out of order, so the only wait there is is "all of them"
                        // (lgkmcnt(0)).  The empty asm makes the next fetch's address depend on the set about to
                        // be consumed: the wait lands BEFORE that fetch is issued, where nothing is in flight but
                        // loads that had a whole group's math to land.  (Not volatile: a volatile asm counts as a
                        // memory clobber and would turn the scalar loads into vector loads.)  The scheduling
                        // barriers keep each fetch ahead of the math that hides it.
                        asm("" : "+s"(j) : "s"(PA), "s"(GA));
                        const v16f PB = src_load<v16f, SRC_CONSTANT>(sp + 2 * (size_t)(j + 8));
                        const v8f GB = src_load<v8f, SRC_CONSTANT>(sg + j + 8);
                        __builtin_amdgcn_sched_barrier(0);
                        interact8<K, true>(R, PA, GA);
                        __builtin_amdgcn_sched_barrier(0);
                        j = min(j + 16, j_last);
                        asm("" : "+s"(j) : "s"(PB), "s"(GB));
                        PA = src_load<v16f, SRC_CONSTANT>(sp + 2 * (size_t)j);
                        GA = src_load<v8f, SRC_CONSTANT>(sg + j);
                        __builtin_amdgcn_sched_barrier(0);
                        interact8<K, true>(R, PB, GB);
                    }
                    g += 2 * pairs;
                    if (pairs == to_close) R.close_chunk();
                }
                if (g < groups) interact8<K, true>(R, PA, GA);  // odd count: the last refill fetched it
                j = j_last + 8;
            }
            for (; j < j_end; j++) interact<K, true>(R, f2v{sp[2 * (size_t)j], sp[2 * (size_t)j + 1]}, sg[j]);
        }
        // a short last block: anything after the last multiple of 256 sources of this slice (same blocks as the
        // LDS variant, whose last tile may be padded)
        if ((v_hi - v_lo) & (CHUNK * CLOSE_EVERY - 1)) R.close_chunk();
    }

    // ---- combine the W slices in wave order, integrate, store -------------------------------------------
    auto finish = [&](uint32_t logical, float sx, float sy) {
        if (p.split > 1) {
            if (logical < p.n_recv) {
                float2 *slot = &p.parts[(size_t)part_y * p.n_recv + logical];
                if constexpr (FUSED) {
                    // agent-scope relaxed store (one 8-byte access): written through to the point every XCD's loads of the
                    // same scope read
                    const uint64_t bits = (uint64_t)__float_as_uint(sx) | ((uint64_t)__float_as_uint(sy) << 32);
                    __hip_atomic_store(reinterpret_cast<uint64_t *>(slot), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    *slot = make_float2(sx, sy);
                }
            }
        } else {
            finish_receiver(p, logical, sx, sy, dt);
        }
    };

    if constexpr (W == 1) {
#pragma unroll
        for (int k = 0; k < K; k++) finish(recv_base + k * WAVE + lane, R.s[k].x, R.s[k].y);
    } else {
#pragma unroll
        for (int k = 0; k < K; k++) partial[wid][k * WAVE + lane] = make_float2(R.s[k].x, R.s[k].y);
        __syncthreads();
#pragma unroll
        for (uint32_t slot = tid; slot < WAVE * K; slot += WAVE * W) {
            const float2 a = wave_sum(&partial[0][slot], WAVE * K, W);
            finish(recv_base + slot, a.x, a.y);
        }
    }

    if constexpr (FUSED) {
        // EVERY workgroup must reach this tail: there is no early return anywhere above, and none may be added -- a
        // workgroup that left without drawing its ticket would leave its tile unfinished in this launch and the ticket
        // non-zero for the next (the host re-zeroes the tickets at every upload and chain build, step_chain.hip zero_tickets).
        // The last workgroup of this receiver tile to get here adds the parts, in part order like finish_kernel, and
        // integrates.  Every thread's part stores have been acknowledged (vmcnt(0)) before the workgroup takes its ticket;
        // the last arriver therefore finds all parts written, and reads them with the same scope they were written with.
        if (p.split > 1) {
            __shared__ uint32_t is_last;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                const uint32_t t = __hip_atomic_fetch_add(&p.tickets[tile_x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                is_last = t == p.split - 1 ? 1u : 0u;
                if (is_last) __hip_atomic_store(&p.tickets[tile_x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next launch
            }
            __syncthreads();
            if (is_last) {
                for (uint32_t slot = tid; slot < WAVE * K; slot += WAVE * W) {
                    const uint32_t logical = recv_base + slot;
                    if (logical >= p.n_recv) continue;
                    // like finish_kernel: every part load issued before the first use (unused slots re-read the last part
                    // and are dropped by a select), or the loads would queue up behind each other's round trips
                    float2 part[MAX_SPLIT];
#pragma unroll
                    for (uint32_t s = 0; s < (uint32_t)MAX_SPLIT; s++) {
                        const uint64_t bits = __hip_atomic_load(reinterpret_cast<const uint64_t *>(&p.parts[(size_t)(s < p.split ? s : p.split - 1) * p.n_recv + logical]),
                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        part[s] = make_float2(__uint_as_float((uint32_t)bits), __uint_as_float((uint32_t)(bits >> 32)));
                    }
                    // the integrator's state rides the same round trip (finish_receiver would fetch it behind the sums)
                    const uint32_t i = receiver_slot(p, logical);
                    const float2 a0 = p.acc[i], v0 = p.vel[i], q0 = p.pos_in[i];
                    float sx = 0.0f, sy = 0.0f;
#pragma unroll
                    for (uint32_t s = 0; s < (uint32_t)MAX_SPLIT; s++) add_part(sx, sy, part[s], s < p.split);
                    finish_loaded(p, i, make_float2(sx, sy), a0, v0, q0, dt);
                }
            }
        }
    }
