"""What the reads kinds of tests/sequence_driver.py and tests/world_sequence.py call with, at the scale of gpu_common.synth's
worlds (normal, sigma 1e4): the factories of sequence_driver.Env for probes, views, edges, centres and the radius, and the
assertion that these arguments give the calls something to say.  A plain helper module (TEST INFRASTRUCTURE)."""
import numpy as np

import nbody_amd as nb
import neighbour_ref as nref
import paircount_ref as pref
import sequence_driver as sd

RADIUS = 600.0                     # a few neighbours inside it in the middle of a world, none at its rim
R_MIN, R_MAX = 500.0, 1.5e4        # the edges of profile and pair_counts: particles and pairs inside, between and beyond them
MOST_MEMBERS = 12
_probe_sets = np.random.default_rng(78).standard_normal((2, MOST_MEMBERS, max(sd.POINT_COUNTS), 2)).astype(np.float32) * 1.0e4
_CENTRES = (((1000.0, -2000.0), (3.0, -1.5)), ((-3000.0, 500.0), (-2.0, 4.0)))


def edges(bins):
    return nb.profile_edges(R_MIN, R_MAX, bins)


def assert_the_reads_have_something_to_say(worlds):
    """worlds: [(particles, mass_len)].  With the numpy models on these states: the radius leaves some receivers with a count of
    zero and some with a positive one, and the edges leave at least two bins non-empty and at least one pair outside them -- a
    call that returned all zeros would not pass.  (The third output of pair_counts, the pairs whose separation is NaN, is zero
    for every finite state, and the sequences rest on finite states: "outside the edges" is rows 0 and bins + 1 of the table.)"""
    counts = np.concatenate([nref.model(part, m, radius=RADIUS)[2] for part, m in worlds])
    assert (counts == 0).any() and (counts > 0).any(), "the radius does not split the receivers"
    most = max(sd.BINS)          # every pair is evaluated once, at the finest edges; the coarser ones are every k-th of them
    fine = edges(most)
    table = sum(pref.model(part, m, fine, pref.MM)[0][:, 0] for part, m in worlds if m >= 2)
    for bins in sd.BINS:
        assert np.array_equal(edges(bins), fine[::most // bins])
        inner = table[1:-1].reshape(bins, most // bins).sum(axis=1)
        assert np.count_nonzero(inner) >= 2 and table[0] + table[-1] > 0, f"{bins} bins: the edges do not spread the pairs"


def factories(members, view=None):
    """keyword arguments for sequence_driver.Env / world_sequence.Env: view (w, h) is `view` where one is given, member b's own
    view looks at another place; two probe sets and two centres, each one for all members or one per member"""
    assert members <= MOST_MEMBERS

    def points(count, which=0, per_member=False):
        return _probe_sets[which][:members, :count] if per_member else _probe_sets[which][0, :count]

    def the_view(w, h, b=None):
        if b is None and view is not None:
            return view(w, h)
        b = b or 0
        return nb.RenderView.make((500.0 * b, -300.0 * b), (w / 2, h / 2), w / 6.0e4, w, h, 2.0e4)

    def centre(which, per_member=False):
        c, u = (np.array(x, dtype=np.float32) for x in _CENTRES[which])
        if not per_member:
            return c, u
        shift = np.arange(members, dtype=np.float32)[:, None]
        return c + 100.0 * shift, u - 0.125 * shift
    return dict(view=the_view, points=points, edges=edges, centre=centre, radius=RADIUS)
