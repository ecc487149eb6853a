"""The launch walk of an ensemble's fixed Euler steps (nbody_amd/csrc/ensemble_walk.h), without a GPU.

walk_ensemble is a host template over a target and a table of launch groups; batch.hip's StepTarget is its target in the
library, for uniform ensembles (one group) and ragged ones alike.  Here a recording target prints what it is asked to launch,
in a stand-alone program built with the address and undefined-behaviour sanitizers, and the sequences are compared with the
ones spelled out below.  The expected strings are written from the statement of the walk, not from the code:

  n = 0: nothing.  Let cur0 be the phase on entry.  If any lane-split group exists, then for each of the n steps every
  lane-split group, in group order, gets one launch that reads buffer cur and writes cur ^ 1, and then the phase flips once.
  Then every chain group runs its whole call in place in buffer cur0, in launches of at most 65 536 steps.  If the phase now
  differs from cur0, each chain group gets one row copy from cur0 into the current buffer.  The walk returns the launches.

Tokens: L<g>:<in>><out> a lane-split launch of group g, C<g>@<buf>x<steps> a chain launch, R<g>:<from>><to> a row copy; a
line ends in "= <launches returned> cur=<final phase>".  Groups are numbered in table order; c = chain, l = lane-split.
"""
import os
import re
import subprocess

import pytest

import nbody_amd as nb

CSRC = os.path.join(nb.ROOT, "nbody_amd", "csrc")

PROBE_SRC = r'''
#include <stdio.h>
#include <string>
#include <vector>
#include "ensemble_walk.h"

struct Group {
    int path, id;
};

struct Recorder {
    std::string out;
    void lanes(const Group &g, int in) { out += " L" + std::to_string(g.id) + ":" + std::to_string(in) + ">" + std::to_string(in ^ 1); }
    void chain(const Group &g, int buf, uint32_t steps) {
        out += " C" + std::to_string(g.id) + "@" + std::to_string(buf) + "x" + std::to_string(steps);
    }
    void copy(const Group &g, int from, int to) { out += " R" + std::to_string(g.id) + ":" + std::to_string(from) + ">" + std::to_string(to); }
};

#ifdef MUTANT
// the walk as its statement has it, with one mistake: 1 the copy before the chain launches, 2 the phase flips once per group,
// 3 the chain runs in cur, 4 the copy is issued although the phase did not move, 5 the chunk limit is off by one
template <class Groups, class T>
uint32_t walk(T &t, const Groups &groups, int &cur, uint32_t n, uint32_t chunk) {
    uint32_t launches = 0;
    if (n == 0) return 0;
    const int cur0 = cur;
    bool any = false;
    for (const auto &g : groups) any = any || g.path != 0;
    for (uint32_t i = 0; i < n && any; i++) {
        for (const auto &g : groups) {
            if (g.path == 0) continue;
            t.lanes(g, cur);
            launches++;
            if (MUTANT == 2) cur ^= 1;
        }
        if (MUTANT != 2) cur ^= 1;
    }
    if (MUTANT == 5) chunk -= 1;
    for (const auto &g : groups) {
        if (g.path != 0) continue;
        const bool moved = MUTANT == 4 ? true : cur != cur0;
        if (MUTANT == 1 && moved) t.copy(g, cur0, cur), launches++;
        for (uint32_t left = n; left > 0;) {
            const uint32_t steps = left > chunk ? chunk : left;
            t.chain(g, MUTANT == 3 ? cur : cur0, steps);
            left -= steps;
            launches++;
        }
        if (MUTANT != 1 && moved) t.copy(g, cur0, cur), launches++;
    }
    return launches;
}
#else
template <class Groups, class T>
uint32_t walk(T &t, const Groups &groups, int &cur, uint32_t n, uint32_t chunk) { return nbi::walk_ensemble(t, groups, cur, n, chunk); }
#endif

static void run(const char *name, const std::vector<Group> &groups, uint32_t n, int cur) {
    Recorder r;
    const int cur0 = cur;
    const uint32_t launches = walk(r, groups, cur, n, 65536u);
    printf("%s n=%u cur=%d:%s = %u cur=%d\n", name, n, cur0, r.out.c_str(), launches, cur);
}

int main() {
    const std::vector<Group> chain = {{0, 0}}, lane = {{1, 0}}, three = {{0, 0}, {1, 1}, {1, 2}}, two = {{1, 0}, {1, 1}};
    for (uint32_t n : {0u, 3u, 65536u, 65541u}) run("c", chain, n, 0);
    for (int cur = 0; cur < 2; cur++)
        for (uint32_t n = 1; n <= 3; n++) run("l", lane, n, cur);
    for (int cur = 0; cur < 2; cur++)
        for (uint32_t n = 2; n <= 3; n++) run("cll", three, n, cur);
    run("ll", two, 3, 0);
    return 0;
}
'''

# written out by hand from the statement above
EXPECTED = [
    # one chain group: the phase never moves, no copy; 65 536 steps are one launch, 65 541 are 65 536 + 5
    "c n=0 cur=0: = 0 cur=0",
    "c n=3 cur=0: C0@0x3 = 1 cur=0",
    "c n=65536 cur=0: C0@0x65536 = 1 cur=0",
    "c n=65541 cur=0: C0@0x65536 C0@0x5 = 2 cur=0",
    # one lane-split group: one launch per step, the phase flips after each
    "l n=1 cur=0: L0:0>1 = 1 cur=1",
    "l n=2 cur=0: L0:0>1 L0:1>0 = 2 cur=0",
    "l n=3 cur=0: L0:0>1 L0:1>0 L0:0>1 = 3 cur=1",
    "l n=1 cur=1: L0:1>0 = 1 cur=0",
    "l n=2 cur=1: L0:1>0 L0:0>1 = 2 cur=1",
    "l n=3 cur=1: L0:1>0 L0:0>1 L0:1>0 = 3 cur=0",
    # chain + (8, 8) + (16, 4): both lane-split groups read the same buffer within a step; the chain stays in cur0 and is
    # copied over only after an odd number of steps
    "cll n=2 cur=0: L1:0>1 L2:0>1 L1:1>0 L2:1>0 C0@0x2 = 5 cur=0",
    "cll n=3 cur=0: L1:0>1 L2:0>1 L1:1>0 L2:1>0 L1:0>1 L2:0>1 C0@0x3 R0:0>1 = 8 cur=1",
    "cll n=2 cur=1: L1:1>0 L2:1>0 L1:0>1 L2:0>1 C0@1x2 = 5 cur=1",
    "cll n=3 cur=1: L1:1>0 L2:1>0 L1:0>1 L2:0>1 L1:1>0 L2:1>0 C0@1x3 R0:1>0 = 8 cur=0",
    # two lane-split groups, no chain: nothing after the steps
    "ll n=3 cur=0: L0:0>1 L1:0>1 L0:1>0 L1:1>0 L0:0>1 L1:0>1 = 6 cur=1",
]

MUTANTS = {1: "the copy before the chain launches", 2: "the phase flips once per group", 3: "the chain runs in cur",
           4: "the copy although the phase did not move", 5: "the chunk limit off by one"}


def build_and_run(d, mutant=None):
    src = d / "walk_probe.cpp"
    src.write_text(PROBE_SRC)
    exe = str(d / ("probe%s" % (mutant or "")))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, str(src), "-o", exe] + (["-DMUTANT=%d" % mutant] if mutant else []),
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (mutant, r.returncode, r.stderr)
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def probe_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("ensemble_walk")


def test_walk_launches_what_the_statement_says(probe_dir):
    """15 walks: sequence, returned launch count and final phase of each."""
    got = build_and_run(probe_dir)
    assert len(EXPECTED) == 15
    assert got == EXPECTED, "\n".join("%s\n   want %s" % (g, w) for g, w in zip(got, EXPECTED) if g != w)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_expected_sequences_reject_a_wrong_walk(probe_dir, mutant):
    """Teeth: the same walk with one mistake prints a different sequence, and only where the mistake can show."""
    got = build_and_run(probe_dir, mutant)
    wrong = {line.split(":")[0] for line, want in zip(got, EXPECTED) if line != want}
    assert len(got) == 15 and wrong, MUTANTS[mutant]
    if mutant in (1, 3):        # only where a chain group met a phase that moved
        assert wrong == {"cll n=3 cur=0", "cll n=3 cur=1"}
    elif mutant == 2:           # only with two lane-split groups
        assert {w.split()[0] for w in wrong} == {"cll", "ll"} and len(wrong) == 5
    elif mutant == 4:           # every chain walk of n > 0 whose phase stayed
        assert wrong == {"c n=3 cur=0", "c n=65536 cur=0", "c n=65541 cur=0", "cll n=2 cur=0", "cll n=2 cur=1"}
    else:                       # only calls of at least 65 536 steps
        assert wrong == {"c n=65536 cur=0", "c n=65541 cur=0"}


def test_the_header_stands_alone_and_the_library_walks_with_it():
    """No HIP include and no state of its own; batch.hip steps through it and through nothing else, with the chunk of the statement."""
    text = open(os.path.join(CSRC, "ensemble_walk.h")).read()
    assert re.findall(r"#include\s+(\S+)", text) == ["<stdint.h>"] and "static " not in text
    batch = open(os.path.join(CSRC, "batch.hip")).read()
    assert '#include "ensemble_walk.h"' in batch
    assert len(re.findall(r"walk_ensemble\(\w+, s->groups, s->cur, n, CHAIN_MAX_STEPS_PER_LAUNCH\)", batch)) == 2
    assert "launch_lane_steps" not in batch and "launch_ragged_steps" not in batch
    assert "CHAIN_MAX_STEPS_PER_LAUNCH = 1u << 16;" in open(os.path.join(CSRC, "pipeline_internal.h")).read()   # the probe's 65536u
