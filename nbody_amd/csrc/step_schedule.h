// step_schedule.h -- the launch schedule of the device-chosen and the leapfrog step calls, written once.  No HIP, no state:
// the target says what a launch is (step_schedule.hip for a SimPipeline, batch.hip for a SimBatch), this says which and when.
//
//   adaptive Euler      [zero the step word, one step]  mark  { criterion -> step word, step } x n                    mark
//   fixed leapfrog      zero the step word, [one force]  mark  { kicks(close i > 0, open; row 0), force } x n  close   mark
//   adaptive leapfrog   the same with a criterion -> kick word i & 1 before every pass, which closes step i - 1 with the
//                       other word and opens step i with this one; the last pass closes with word (n - 1) & 1
//
// The step word is what the step kernels read as dt: 0 for a whole leapfrog call (its launches are force evaluations), the
// criterion's choice per Euler step.  [..] = priming: Euler when asked for (NB_ADAPT_PRIME), leapfrog whenever acc is not
// the state's own.  Callers return before n = 0 reaches this.
#pragma once

#include <stdint.h>

namespace nbi {

struct Schedule {
    uint32_t n;
    bool leapfrog, adaptive;
    bool prime;   // Euler only
};

// T: acc_current(), zero_step_word(), force() (the launches of a one-step update reading the step word, phase flip included),
// criterion(i, row) (row < 0: into the step word), kicks(close, open, close_row, open_row), begin_mark(), end_mark()
template <class T>
void run_schedule(T &t, Schedule c) {
    const bool prime = c.leapfrog ? !t.acc_current() : c.prime;
    if (c.leapfrog || prime) t.zero_step_word();
    if (prime) t.force();
    t.begin_mark();
    for (uint32_t i = 0; i < c.n; i++) {
        const uint32_t row = c.adaptive ? i & 1 : 0, other = c.adaptive ? row ^ 1 : 0;
        if (c.adaptive) t.criterion(i, c.leapfrog ? (int)row : -1);
        if (c.leapfrog) t.kicks(i > 0, true, other, row);
        t.force();
    }
    if (c.leapfrog) t.kicks(true, false, c.adaptive ? (c.n - 1) & 1 : 0, 0);
    t.end_mark();
}

}  // namespace nbi
