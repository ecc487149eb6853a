// step_schedule.hip -- device-chosen and leapfrog steps of a SimPipeline: what the launches of step_schedule.h's one schedule
// are for one world, and the records a call leaves behind.  Everything goes on the pipeline's stream and nothing returns to
// the host between the steps.  Kernels: timestep.hip (the criterion), leapfrog.hip (the kick / drift passes); the force
// launches are those of a one-step dt = 0 update (step_chain.hip launch_step).  The C-ABI entry points of both step kinds
// (include/nbody_adaptive.h, include/nbody_leapfrog.h) are at the end.
#include "pipeline_internal.h"
#include "leapfrog.h"
#include "step_schedule.h"
#include "timestep.h"
#include "timestep_common.h"

namespace nbi {

// One device buffer per pipeline (SimPipeline::adapt): ADAPT_HEAD bytes of records -- the AdaptState of the call at 0, of
// nb_hip_timestep at 32, its result at 64, the two step-size words of the leapfrog passes at LEAPFROG_WORDS -- then the log.
constexpr size_t ADAPT_HEAD = 128;
constexpr size_t LEAPFROG_WORDS = 96;

void check_adaptive_cfg(const void *s, uint32_t n, const NbAdaptive *cfg, const char *what) {
    NB_ASSERT(s != nullptr && cfg != nullptr, "%s: NULL argument", what);
    const char *fault = nb_timestep_cfg_fault(cfg);
    NB_ASSERT(fault == nullptr, "%s: %s (eta %g, dt_min %g, dt_max %g, span %g)", what, fault, (double)cfg->eta, (double)cfg->dt_min,
              (double)cfg->dt_max, cfg->span);
    NB_ASSERT(n <= NB_ADAPT_MAX_STEPS, "%s: %u steps > 2^20 in one call", what, n);
}

namespace {

// the checks abort on a bad call before anything touches a device
void check_adaptive(const SimPipeline *s, uint32_t n, const NbAdaptive *cfg, const char *what) {
    check_adaptive_cfg(s, n, cfg, what);
    NB_ASSERT(!s->sharded, "%s of a sharded pipeline needs a collective over the ranks: not supported", what);
    NB_ASSERT(n == 0 || s->on_device, "%s before SetSimulationData", what);
}

void check_leapfrog(const SimPipeline *s, uint32_t n, const char *what) {
    NB_ASSERT(s != nullptr, "%s: NULL argument", what);
    NB_ASSERT(!s->sharded, "%s of a sharded pipeline needs a collective over the ranks: not supported", what);
    NB_ASSERT(n == 0 || s->on_device, "%s before SetSimulationData", what);
}

// the head and room for `log` step sizes; a regrow carries the head over (a continued call goes on from its records)
void grow_adapt(SimPipeline *s, size_t log) {
    s->adapt.grown_carrying(s->stream, ADAPT_HEAD + (log < 64 ? 64 : log) * sizeof(float), ADAPT_HEAD);
}

// One world as the schedule's target.  The step word is dt_dev; the two kick words sit in the adaptive head.
struct PipelineTarget {
    SimPipeline *s;
    nb::LaunchShape sh;
    nb::TimestepParams p;   // adaptive calls only
    float *log;
    float *words;
    uint32_t forces = 0;

    bool acc_current() const { return s->acc_current; }
    void zero_step_word() { upload_dt(s, 0.0f); }
    // what a one-step dt = 0 update launches (an Euler step: the same launches, reading the criterion's choice)
    void force() {
        launch_step(s, sh, whole_step(s, s->cur, 0.0f), s->stream);
        s->cur ^= 1;
        forces++;
    }
    void criterion(uint32_t i, int row) {
        p.log = log + i;
        p.dt_out = row < 0 ? s->dt_dev : words + row;
        nb::launch_timestep(s->stream, p);
    }
    void kicks(bool close, bool open, uint32_t close_row, uint32_t open_row) {
        nb::LeapfrogParams lf;
        memset(&lf, 0, sizeof lf);
        // the latest positions; an unsharded pipeline's sources are this array itself (whole_step: src_pos[b] == pos[b]), so the
        // drift leaves no second copy behind
        lf.pos = s->pos[s->cur];
        lf.vel = s->vel;
        lf.acc = s->acc;
        lf.n = s->n_real;
        lf.dt_close = words + close_row;
        lf.dt_open = words + open_row;
        nb::launch_leapfrog(s->stream, lf, close, open, 0);
    }
    void begin_mark() {
        if (s->timing) s->step_iv.begin(s->stream);
    }
    void end_mark() { ASSERT_HIP(hipGetLastError(), "step launches (%u particles)", s->n_real); }
};

// One call of the schedule and every record it leaves: the only place these fields are set for a device-chosen or leapfrog call.
void run_call(SimPipeline *s, Schedule c, const nb::TimestepParams &p, float *log) {
    PipelineTarget t = {s, resolve_shape(s), p, log, reinterpret_cast<float *>(s->adapt + LEAPFROG_WORDS)};
    if (c.leapfrog) s->lf_primed = !s->acc_current;
    run_schedule(t, c);
    if (c.leapfrog) s->lf_force_launches = t.forces;
    end_call(s, c.n * passes_for(s, whole_step(s, s->cur, 0.0f)));
    s->dt_valid = false;            // the step word holds 0 or the device's last choice: the next fixed-step call uploads its own
    s->acc_current = c.leapfrog;    // Euler steps leave the acc of the state before them
}

// per step the criterion launch, then the launches of a one-step call without its dt upload; enqueue only
void enqueue_adaptive(SimPipeline *s, uint32_t n, const NbAdaptive *cfg) {
    s->adapt_logged = 0;
    if (s->slots == 0 || n == 0) return;
    use_device();
    grow_adapt(s, n);
    begin_call(s);
    char *head = s->adapt;
    nb::TimestepParams p = nb::timestep_params(s->acc, s->radius, s->n_real, 0, *cfg);
    p.state = reinterpret_cast<nb::AdaptState *>(head);
    p.commit = 1;
    if (!(cfg->flags & NB_ADAPT_CONTINUE) || !s->adapt_armed) nb::launch_arm(s->stream, p.state, 1);
    s->adapt_armed = true;
    const bool leapfrog = (cfg->flags & NB_ADAPT_LEAPFROG) != 0;
    run_call(s, {n, leapfrog, true, !leapfrog && (cfg->flags & NB_ADAPT_PRIME) != 0}, p, reinterpret_cast<float *>(head + ADAPT_HEAD));
    s->adapt_logged = n;
}

// n kick-drift-kick steps of one size
void enqueue_leapfrog(SimPipeline *s, uint32_t n, float dt) {
    if (s->slots == 0 || n == 0) return;
    use_device();
    grow_adapt(s, 0);
    begin_call(s);
    nb::launch_set_scalar(s->stream, reinterpret_cast<float *>(s->adapt + LEAPFROG_WORDS), dt);
    run_call(s, {n, true, false, false}, nb::TimestepParams{}, nullptr);
}

void enqueue_timestep_peek(SimPipeline *s, const NbAdaptive *cfg) {
    use_device();
    grow_adapt(s, 0);
    char *head = s->adapt;
    nb::TimestepParams p = nb::timestep_params(s->acc, s->radius, s->n_real, 0, *cfg);
    p.state = reinterpret_cast<nb::AdaptState *>(head + sizeof(nb::AdaptState));
    p.dt_out = reinterpret_cast<float *>(head + 2 * sizeof(nb::AdaptState));
    p.commit = 0;
    nb::launch_arm(s->stream, p.state, 1);
    nb::launch_timestep(s->stream, p);
    ASSERT_HIP(hipGetLastError(), "timestep_kernel launch (%u particles)", s->n_real);
}

}  // namespace

}  // namespace nbi

using namespace nbi;

extern "C" {

// ---- adaptive steps (include/nbody_adaptive.h; kernels: timestep.hip) ----------------------------------------------------

void nb_hip_adaptive_steps_async(SimPipeline *s, uint32_t n, const NbAdaptive *cfg) {
    check_adaptive(s, n, cfg, "nb_hip_adaptive_steps_async");
    enqueue_adaptive(s, n, cfg);
}

void nb_hip_adaptive_collect(SimPipeline *s, float *dt_log, NbAdaptiveResult *out) {
    NB_ASSERT(s != nullptr, "nb_hip_adaptive_collect: NULL pipeline");
    if (out) memset(out, 0, sizeof *out);
    const uint32_t n = s->adapt_logged;
    if (n == 0 || !s->on_device) return;
    use_device();
    const size_t bytes = ADAPT_HEAD + (dt_log ? (size_t)n * sizeof(float) : 0);
    s->adapt_host.resize(bytes);
    ASSERT_HIP(hipMemcpyAsync(s->adapt_host.data(), s->adapt, bytes, hipMemcpyDeviceToHost, s->stream), "D2H of %u step sizes and the result", n);
    nb_hip_sync(s);
    if (out) *out = nb::adaptive_result(s->adapt_host.data());
    if (dt_log) memcpy(dt_log, s->adapt_host.data() + ADAPT_HEAD, (size_t)n * sizeof(float));
}

void nb_hip_adaptive_steps(SimPipeline *s, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out) {
    check_adaptive(s, n, cfg, "nb_hip_adaptive_steps");
    enqueue_adaptive(s, n, cfg);
    nb_hip_adaptive_collect(s, dt_log, out);
}

void nb_hip_timestep(SimPipeline *s, const NbAdaptive *cfg, float *dt) {
    check_adaptive(s, 1, cfg, "nb_hip_timestep");
    NB_ASSERT(dt != nullptr, "nb_hip_timestep: NULL result");
    if (s->slots == 0) {
        *dt = cfg->dt_max;
        return;
    }
    enqueue_timestep_peek(s, cfg);
    ASSERT_HIP(hipMemcpyAsync(dt, s->adapt + 2 * sizeof(nb::AdaptState), sizeof(float), hipMemcpyDeviceToHost,
                              s->stream),
               "D2H of the step size");
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_timestep");
}

// ---- leapfrog steps (include/nbody_leapfrog.h; kernels: leapfrog.hip) ----------------------------------------------------

void nb_hip_leapfrog_steps_async(SimPipeline *s, uint32_t n, float dt) {
    check_leapfrog(s, n, "nb_hip_leapfrog_steps_async");
    enqueue_leapfrog(s, n, dt);
}

void nb_hip_leapfrog_steps(SimPipeline *s, uint32_t n, float dt) {
    check_leapfrog(s, n, "nb_hip_leapfrog_steps");
    enqueue_leapfrog(s, n, dt);
    if (n > 0) nb_hip_sync(s);
}

void nb_hip_last_leapfrog_info(const SimPipeline *s, uint32_t *force_launches, int *primed) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    if (force_launches) *force_launches = s->lf_force_launches;
    if (primed) *primed = s->lf_primed ? 1 : 0;
}

}  // extern "C"
