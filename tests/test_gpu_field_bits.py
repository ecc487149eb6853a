"""The bits of the field sampler against the digests recorded on an MI355X (tests/golden/field_bits.json, written by
tools/record_field_bits.py; its header names the commit that produced it): Phi and g, both kernel shapes, probes and a map,
on the smallest worlds and sample counts at which the summation order can go wrong.  The other field tests prove split == wave
and closeness to float64; an edit that moves both shapes' bits together shows only here."""
import json
import os
import sys

import pytest

import nbody_amd as nb

sys.path.insert(0, os.path.join(nb.ROOT, "tools"))
import record_field_bits as rec  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_cell_of_the_grid_has_the_recorded_bits():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    with open(os.path.join(nb.ROOT, "tests", "golden", "field_bits.json")) as f:
        want = json.load(f)
    worlds, view, soft = rec.inputs()
    assert soft == want["softening"] and rec.input_digests(worlds) == want["inputs"], "inputs differ, regenerate"
    got = rec.result_digests(worlds, view, soft)
    assert sorted(got) == sorted(want["results"]) and len(got) == 5 * 2 * 2 * 4
    wrong = sorted(k for k in got if got[k] != want["results"][k])
    assert not wrong, f"{len(wrong)} of {len(got)} cells differ from commit {want['recorded_from_commit'][:7]}'s bits: {wrong[:8]}"
