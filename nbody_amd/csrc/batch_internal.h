// batch_internal.h -- struct SimBatch and what batch.hip (life cycle, stepping, traces) and batch_observe.hip (the read-only
// calls) share.  C++, not part of the C-ABI.
//
// Every device array and event of a SimBatch is a member of an owner type (pipeline_internal.h DevBuf / Interval): made by
// materialize or on a call's first use, released by the member's destructor when nb_hip_batch_destroy deletes the struct,
// after it has drained the stream.  nb_hip_batch_destroy itself only syncs and destroys the stream.  Every read-only call, the
// renders included, shares one scratch and one host protocol with those of a pipeline: pipeline_internal.h ReadScratch / read_call.
#pragma once

#include "pipeline_internal.h"

struct SimBatch {
    uint32_t count = 0;     // members
    uint32_t n = 0;         // particles per member; ragged: of the largest member
    uint32_t stride = 0;    // rows per member in the SoA arrays: n rounded up to 64 (256-byte aligned float rows)
    std::vector<uint32_t> n_len;      // [count] particles of each member
    std::vector<uint64_t> offsets;    // [count + 1] member b's first record in the packed AoS arrays of the seam
    bool ragged = false;              // made by nb_hip_ragged_create
    std::vector<uint32_t> mass_len;   // [count]
    std::vector<float> dt_host;       // [count]: what dt_dev holds (valid once dt_valid)
    bool dt_valid = false;
    uint32_t dt_uploads = 0;

    bool on_device = false;
    bool has_data = false;
    hipStream_t stream = nullptr;
    nbi::Interval step_iv;   // around the launches of the last update
    nbi::DevBuf<float2> pos[2];
    nbi::DevBuf<float2> vel, acc;
    nbi::DevBuf<float> radius, mass, gm;
    nbi::DevBuf<uint32_t> mass_len_dev;
    nbi::DevBuf<float> dt_dev;
    nbi::DevBuf<Particle> aos;   // device staging of Set / Get: [count][n] Particle
    int cur = 0;           // pos[cur] is the latest state (the chain path never moves it)

    // The launch shape, fixed at creation: the launch groups, in the order chain, lane-split (8, 8), lane-split (16, 4); those
    // without members are absent.  A uniform ensemble is one group of all members.  `ragged` says only how the launches
    // find the members: by block index, or through n_len_dev and the groups' lists (null in a uniform ensemble).
    struct Group {
        int path = 0, k = 2, w = 16, lanes = 1;   // path: 0 chain, 1 lane-split; chain: w of the group's largest member
        uint32_t tiles = 0;                       // chain: chain_tiles(max_n)
        uint32_t max_n = 0;                       // its largest member
        uint32_t workgroups = 0;                  // per launch
        std::vector<uint32_t> members;            // ascending member indices
        nbi::DevBuf<uint32_t> list;               // ragged: the same on the device
        const void *fn = nullptr;                 // lane-split: the kernel, the grid, the block and the LDS bytes of a launch
        dim3 grid, block;
        size_t lds = 0;
    };
    std::vector<Group> groups;
    // some group is lane-split (the chain group comes first): both position buffers exist, traces interleave
    bool lane_split() const { return groups.back().path != 0; }
    nbi::DevBuf<uint32_t> n_len_dev;     // ragged only, like offsets_dev
    nbi::DevBuf<uint64_t> offsets_dev;

    // every read-only call (all of batch_observe.hip, nb_hip_ensemble_profile, nb_hip_ensemble_pair_counts, nb_hip_ensemble_neighbours, nb_hip_ensemble_groups):
    // their scratch, and the interval of all but bounds and the renders (pipeline_internal.h ReadScratch)
    nbi::ReadScratch read;
    // the energy slab stays a member of its own: traced updates (batch.hip) write it too, and they are no read-only calls
    nbi::DevBuf<double> diag;      // float64 slab: [count][tiles of 128][NB_DIAG_SUMS] + the [count][NB_DIAG_SUMS] results

    // nb_hip_ensemble_trace: the rows of the last traced call, on the device and on their way to WorldEnergy
    nbi::DevBuf<double> trace;     // [records][count][NB_DIAG_SUMS]
    std::vector<double> trace_host;
    int trace_mode = 0;          // tuning hook: 1 = interleaved diagnostics launches also where the chain could record
    int trace_fused = 0;         // what the last traced call did
    uint32_t trace_launches = 0;

    // nb_hip_ensemble_bounds / _render_counts / _render_rgba (kernels: render_kernels.hip): an interval of their own
    nbi::Interval render_iv;
    int render_mode = 0;                     // tuning hook: 1 = the global path also where the tile path applies
    int render_tile = 0;                     // what the last render did (a bounds call leaves both alone)
    uint32_t render_launches = 0;

    // nb_hip_ensemble_adaptive_steps (kernels: timestep.hip): [count] AdaptState, then the call's log [n][count]; grown on demand
    nbi::DevBuf<char> adapt;
    bool adapt_armed = false;   // the records hold a call to continue (NB_ADAPT_CONTINUE)
    std::vector<char> adapt_host;

    // leapfrog steps (kernels: leapfrog.hip): the step sizes of the kick / drift passes, [2][count] -- a fixed-step call uses
    // the first row, an adaptive one alternates so that one launch can close step i - 1 and open step i
    nbi::DevBuf<float> lf_dt;
    bool acc_current = false;        // acc = F(x) of the state held: true after a leapfrog call, false after anything else that moves it
    uint32_t lf_force_launches = 0;  // force evaluations of the last leapfrog call (nb_hip_ensemble_last_leapfrog_info)
    bool lf_primed = false;          // ... and whether it had to run one first
};

namespace nbi {

// batch_observe.hip, used by traces too: the slab of per-tile rows with room for one call's results behind it, and the two
// launches of an energy diagnostic of the latest state: every member's eight sums -> res[count][NB_DIAG_SUMS]
double *energy_slab(SimBatch *s);
void launch_energy_sums(SimBatch *s, double *res);

}  // namespace nbi
