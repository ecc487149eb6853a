// ensemble_walk.h -- the launches of n fixed Euler steps of an ensemble, written once.  No HIP, no state: the target says
// what a launch is (batch.hip), this says which and when.  The members fall into launch groups (batch_internal.h), chain or
// lane-split; a uniform ensemble is the one-group case.
//
//   lane-split groups   per step one launch each, in group order, from position buffer cur into cur ^ 1; then cur flips, once
//   chain groups        after that the whole call in place in the buffer cur had on entry, at most `chunk` steps per launch;
//                       when cur has moved, one copy of the group's position rows into the buffer that is now the latest,
//                       so that every reader finds all members in pos[cur]
#pragma once

#include <stdint.h>

namespace nbi {

// G: path (0 chain, else lane-split).  T: lanes(g, in) (one step, buffer in -> in ^ 1), chain(g, buf, steps), copy(g, from, to).
// Returns the launches made.
template <class Groups, class T>
uint32_t walk_ensemble(T &t, const Groups &groups, int &cur, uint32_t n, uint32_t chunk) {
    uint32_t launches = 0;
    const int cur0 = cur;
    bool lanes = false;
    for (const auto &g : groups) lanes = lanes || g.path != 0;
    for (uint32_t i = 0; i < n && lanes; i++) {
        for (const auto &g : groups) {
            if (g.path == 0) continue;
            t.lanes(g, cur);
            launches++;
        }
        cur ^= 1;
    }
    for (const auto &g : groups) {
        if (g.path != 0) continue;
        for (uint32_t left = n, steps; left > 0; left -= steps, launches++) {
            steps = left > chunk ? chunk : left;
            t.chain(g, cur0, steps);
        }
        if (cur != cur0) {
            t.copy(g, cur0, cur);
            launches++;
        }
    }
    return launches;
}

}  // namespace nbi
