"""The mask range [lo, hi) of a groups call at every edge of group_pairs_kernel's walk: the case table tests/test_group_edges_cpu.py
(the premise, on the CPU, from the model alone) and tests/test_gpu_group_edges.py share.  A plain helper module.

The walk cuts the range at tiles of 128 receivers, blocks of 256 sources, slices of 32 and fetches of 8; its own index arithmetic
is r0 & ~127, r0 / 256 + blockIdx.y * span, j0 = max(first, r0), s1 = min(r1, rb + 128) and the single sources up to the first
multiple of 8.  One world of N = 520 (source blocks of 256, 256 and 8; five receiver tiles, the last of 8) whose mass_len stands
on, before and behind each of those edges, under the three masks and two linking lengths.

An edge is only tested where a link crosses it, so links are PLANTED: particles are moved to sites far from the seeded world
(paircount_ref.world, spread 3) and from one another, where they stand in chains of spacing 0.75 l (l the case's linking length):
neighbours along a chain link, any two others of a site are at least 1.29 l apart and do not.  Every planted link is therefore a
bridge of the link graph -- withhold it and a label changes -- which is what the premise test asserts.  The spacing has to follow
the length: a chain a - b - c whose ends do not link at 2 l while its neighbours link at l contradicts the triangle inequality.

Planted, where they lie inside the range:
  lo with lo + 1, lo with a particle two tiles on, hi - 1 with lo      three chains leaving the site of lo at 0, 120 and 240 degrees
  hi - 1 with hi - 2                                                   the third of them goes on: lo, hi - 1, hi - 2, ...
  e - 1 with e, e the first multiple of 8, 32, 128 and 256 behind lo and the last one before hi       a chain of its own per run
A planted particle must carry a bridge both as a source (j = s < i) and as a receiver, so every chain is extended by a HELPER at
each end that needs one: the next free index above (below) the chain's last planted particle.  Helpers are not held to the
premise; lo has no pair as a receiver and hi - 1 none as a source, whatever the world."""
import numpy as np

import group_ref as gr
from paircount_ref import world

N = 520
MASS_LENS = (7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 519)
LENGTHS = tuple(gr.length_for(N, b=b) for b in (1.0, 2.0))
SPANS = (0, 1, 2)          # nb_hip_group_span: auto, and the two forced lengths whose offsets start from r0 / 256
TILE, BLOCK = 128, 256
SPACING = 0.75          # of the linking length, along a chain
SITE0, SITE_STEP = (60.0, 40.0), 12.0          # the seeded world lies within about +-15; a site is a few linking lengths wide

RAGGED = ((520, 520, 385, 257, 129, 9), (129, 256, 257, 128, 8, 8))          # sizes, mass lengths
UNIFORM = (520, (127, 128, 129, 255, 256, 257))


def edges_of(lo, hi):
    """The multiples e of 8, 32, 128 and 256 next to lo and next to hi with e - 1 and e both inside [lo, hi)."""
    out = set()
    for k in (8, 32, 128, 256):
        first, last = (lo // k + 1) * k, ((hi - 1) // k) * k          # the first with e - 1 >= lo, the last with e < hi
        out |= {e for e in (first, last) if lo <= e - 1 and e < hi}
    return sorted(out)


def plan(lo, hi):
    """(chains, planted): chains = [(site, ray, [indices in order])], consecutive indices of a chain link; planted = the sorted
    indices held to the premise.  Rays 0, 1, 2 leave the site's centre, where the chain's first index stands."""
    if hi - lo < 7:
        return [], []
    marked = set()
    for e in edges_of(lo, hi):
        marked |= {e - 1, e}
    used, chains = set(), []

    def free(x, step):
        x += step
        while lo <= x < hi and x in used:
            x += step
        return x if lo <= x < hi else None

    def run(start, step):
        """start, then its neighbours in direction `step` while they are marked, then one helper."""
        out = [start]
        while lo <= out[-1] + step < hi and out[-1] + step in marked and out[-1] + step not in used:
            out.append(out[-1] + step)
        used.update(out)
        helper = free(out[-1], step)
        if helper is not None:
            out.append(helper)
            used.add(helper)
        return out

    used.add(lo)
    up = [lo] + run(lo + 1, +1)                                         # lo with lo + 1, and on
    used.add(hi - 1)
    down = [lo, hi - 1] + run(hi - 2, -1)                               # hi - 1 with lo and with hi - 2, and on
    chains += [(0, 0, up), (0, 2, down)]
    planted = {lo, lo + 1, hi - 1, hi - 2}
    first_tile = lo & ~(TILE - 1)
    for offset in (70, 37, 101, 5):          # a particle of the tile two on: lane 6 of its second half first
        t = first_tile + 2 * TILE + offset
        if t + 1 < hi and t not in used and t + 1 not in used and t not in marked and t + 1 not in marked:
            used.update((t, t + 1))
            chains.append((0, 1, [lo, t, t + 1]))
            planted.add(t)
            break
    site = 1
    rest = sorted(marked - used)
    while rest:
        body = [rest.pop(0)]
        while rest and rest[0] == body[-1] + 1:
            body.append(rest.pop(0))
        used.update(body)
        below, above = free(body[0], -1), free(body[-1], +1)
        assert below is not None and above is not None, (lo, hi, body)
        used.update((below, above))
        chains.append((site, 0, [below] + body + [above]))
        site += 1
    planted |= marked
    flat = [i for site, _, c in chains for i in (c[1:] if site == 0 else c)] + [lo]
    assert len(flat) == len(set(flat)) and planted <= set(flat), (lo, hi, chains)          # one place per particle
    return chains, sorted(planted)


def edge_world(n, m, members, length, seed=0):
    """(particles (n, 8) float32 with exactly m massive in front, planted indices) for the mask `members` and the linking length."""
    a = world(n, m, seed=seed, spread=3.0)
    lo, hi = gr.span(members, n, m)
    chains, planted = plan(lo, hi)
    step = SPACING * float(np.float32(length))
    for site, ray, chain in chains:
        cx, cy = SITE0[0] + SITE_STEP * site, SITE0[1]
        angle = 2.0 * np.pi * ray / 3.0
        for k, i in enumerate(chain):          # a chain's first index stands at the centre (k = 0)
            a[i, 0], a[i, 1] = cx + step * k * np.cos(angle), cy + step * k * np.sin(angle)
    return a, planted


CASES = [(m, members, length) for m in MASS_LENS for members in gr.MASKS for length in LENGTHS]


def withheld(a, m, members, length, s, as_source):
    """The model's labels when every pair with s as its source (j = s < i) -- or as its receiver (i = s > j) -- is withheld."""
    n = a.shape[0]
    x, y = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
    lo, hi = gr.span(members, n, m)
    ii, jj = gr.links(x, y, lo, hi, length)
    keep = (jj != s) if as_source else (ii != s)
    label = gr.propagate(n, ii[keep], jj[keep])
    out = np.full(n, gr.NONE, dtype=np.uint32)
    out[lo:hi] = label[lo:hi].astype(np.uint32)
    return out


def ensemble_states(sizes, mass_lens, members, length):
    return [edge_world(n, m, members, length, seed=100 + b)[0] for b, (n, m) in enumerate(zip(sizes, mass_lens))]
