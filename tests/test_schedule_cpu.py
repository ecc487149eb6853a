"""The launch schedule of the device-chosen and the leapfrog step calls (nbody_amd/csrc/step_schedule.h), without a GPU.

run_schedule is a host template over a target; a SimPipeline and a SimBatch are its two targets in the library.  Here a
recording target prints what it is asked to launch, in a stand-alone program built with the address and undefined-behaviour
sanitizers, and the sequences are compared with the ones spelled out below.  The expected strings are written from the
statement of the three schedules, not from the code:

  adaptive Euler      if prime: zero the step word, one step.  Mark.  Per i: criterion -> step word, step.
  fixed leapfrog      zero the step word; one force if acc is not current.  Mark.  Per i: kicks(close = i > 0, open; word 0),
                      force.  Then a closing pass with word 0.
  adaptive leapfrog   the same, with a criterion -> kick word i & 1 before each pass, which closes with word (i & 1) ^ 1 and
                      opens with word i & 1; the closing pass uses word (n - 1) & 1.

Tokens: Z zero the step word, F force / step, [ and ] the marks, cI>s criterion of step I into the step word, cI>wR into kick
word R, k(cR,oQ) a pass that closes with word R and opens with word Q ('-' = that half is off).
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
#include "step_schedule.h"

using nbi::Schedule;

struct Recorder {
    bool current;
    std::string out;
    bool acc_current() const { return current; }
    void zero_step_word() { out += " Z"; }
    void force() { out += " F"; }
    void criterion(uint32_t i, int row) { out += " c" + std::to_string(i) + (row < 0 ? ">s" : ">w" + std::to_string(row)); }
    void kicks(bool close, bool open, uint32_t close_row, uint32_t open_row) {
        out += " k(" + (close ? "c" + std::to_string(close_row) : std::string("-")) + "," + (open ? "o" + std::to_string(open_row) : std::string("-")) + ")";
    }
    void begin_mark() { out += " ["; }
    void end_mark() { out += " ]"; }
};

#ifdef MUTANT
// the schedule as the three lists state it, with one mistake: 1 swapped word parity, 2 close on i >= 0, 3 no final close,
// 4 prime after the mark
template <class T>
void run(T &t, Schedule c) {
    const bool prime = c.leapfrog ? !t.acc_current() : c.prime;
    if (c.leapfrog || prime) t.zero_step_word();
    if (prime && MUTANT != 4) t.force();
    t.begin_mark();
    if (prime && MUTANT == 4) t.force();
    for (uint32_t i = 0; i < c.n; i++) {
        uint32_t row = c.adaptive ? i & 1 : 0;
        if (MUTANT == 1 && c.adaptive) row ^= 1;
        const uint32_t other = c.adaptive ? row ^ 1 : 0;
        if (c.adaptive) t.criterion(i, c.leapfrog ? (int)row : -1);
        if (c.leapfrog) t.kicks(MUTANT == 2 ? true : i > 0, true, other, row);
        t.force();
    }
    if (c.leapfrog && MUTANT != 3) t.kicks(true, false, c.adaptive ? ((c.n - 1) & 1) ^ (MUTANT == 1) : 0, 0);
    t.end_mark();
}
#else
template <class T>
void run(T &t, Schedule c) { nbi::run_schedule(t, c); }
#endif

int main() {
    const char *kinds[] = {"euler", "euler+prime", "leapfrog", "adaptive-leapfrog"};
    for (int kind = 0; kind < 4; kind++)
        for (uint32_t n = 0; n <= 3; n++)
            for (int current = 1; current >= 0; current--) {
                Recorder r{current != 0, ""};
                run(r, Schedule{n, kind >= 2, kind != 2, kind == 1});
                printf("%s n=%u acc=%d:%s\n", kinds[kind], n, current, r.out.c_str());
            }
    return 0;
}
'''

# per kind and n: the sequence from the first mark on; `before` is the priming in front of it, by whether acc is current
EULER = ["[ ]", "[ c0>s F ]", "[ c0>s F c1>s F ]", "[ c0>s F c1>s F c2>s F ]"]
LEAPFROG = ["[ k(c0,-) ]",
            "[ k(-,o0) F k(c0,-) ]",
            "[ k(-,o0) F k(c0,o0) F k(c0,-) ]",
            "[ k(-,o0) F k(c0,o0) F k(c0,o0) F k(c0,-) ]"]
ADAPTIVE_LEAPFROG = ["[ k(c1,-) ]",
                     "[ c0>w0 k(-,o0) F k(c0,-) ]",
                     "[ c0>w0 k(-,o0) F c1>w1 k(c0,o1) F k(c1,-) ]",
                     "[ c0>w0 k(-,o0) F c1>w1 k(c0,o1) F c2>w0 k(c1,o0) F k(c0,-) ]"]
EXPECTED = []
for kind, body, before in (("euler", EULER, {1: "", 0: ""}),                      # the step word is NOT zeroed without prime
                           ("euler+prime", EULER, {1: "Z F ", 0: "Z F "}),          # whatever acc is
                           ("leapfrog", LEAPFROG, {1: "Z ", 0: "Z F "}),            # one force when acc is not current
                           ("adaptive-leapfrog", ADAPTIVE_LEAPFROG, {1: "Z ", 0: "Z F "})):
    for n in range(4):
        for current in (1, 0):
            EXPECTED.append("%s n=%d acc=%d: %s%s" % (kind, n, current, before[current], body[n]))

MUTANTS = {1: "swapped word parity", 2: "close on i >= 0", 3: "missing final close", 4: "prime after the mark"}


def build_and_run(d, mutant=None):
    src = d / "schedule_probe.cpp"
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
    return tmp_path_factory.mktemp("schedule")


def test_schedule_launches_what_the_three_lists_say(probe_dir):
    """n in {0, 1, 2, 3} x {adaptive Euler, + prime, fixed leapfrog, adaptive leapfrog} x {acc current, not}: 32 sequences."""
    got = build_and_run(probe_dir)
    assert len(EXPECTED) == 32
    assert got == EXPECTED, "\n".join("%s\n   want %s" % (g, w) for g, w in zip(got, EXPECTED) if g != w)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_expected_sequences_reject_a_wrong_schedule(probe_dir, mutant):
    """Teeth: the same loop with one mistake prints a different sequence, and only where the mistake can show."""
    got = build_and_run(probe_dir, mutant)
    wrong = {line.split(":")[0] for line, want in zip(got, EXPECTED) if line != want}
    assert len(got) == 32 and wrong, MUTANTS[mutant]
    kinds = {w.split()[0] for w in wrong}
    if mutant == 1:
        assert kinds == {"adaptive-leapfrog"}
    elif mutant in (2, 3):
        assert kinds == {"leapfrog", "adaptive-leapfrog"}
    else:
        assert wrong == {l.split(":")[0] for l in EXPECTED if ": Z F" in l}


def test_the_header_stands_alone():
    """No HIP include and no state of its own: the probe above compiles it with a host compiler and nothing else."""
    text = open(os.path.join(CSRC, "step_schedule.h")).read()
    assert re.findall(r"#include\s+(\S+)", text) == ["<stdint.h>"] and "static " not in text
    for src in ("step_schedule.hip", "batch.hip"):
        assert '#include "step_schedule.h"' in open(os.path.join(CSRC, src)).read(), src
