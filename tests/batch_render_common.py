"""What the ensemble-render tests share (tests/test_batch_render_cpu.py, tests/test_gpu_batch_render.py): the view kinds, a
custom palette and the hand-made member."""
import numpy as np

import oracle_binding as ob
import render_ref as rr

KINDS = ("fitted", "mixed", "edge", "collapsed", "nothing")
CUSTOM = dict(background=(10, 20, 30, 40), color=((200, 100, 0, 255), (1, 2, 3, 4), (255, 254, 253, 128)), saturation=3)


def make_view(kind, part, width, height):
    """One member's view of a kind.  rr.mixed_view is defined only for a member that holds an ordinary massive particle (it
    centres on one): a member without one is shown through its fitted view instead, in the "mixed" set too."""
    if kind == "mixed" and not np.any((part[:, 6] > 0) & (part[:, 6] < rr.min_gc_mass())):
        kind = "fitted"
    if kind == "fitted":
        return rr.fit_view(part, width, height)
    return {"mixed": rr.mixed_view, "edge": rr.edge_view, "collapsed": rr.collapsed_view, "nothing": rr.empty_view}[kind](part, width, height)


def hand_made():
    """the particles of test_hand_made_edges_and_non_finite_particles (tests/test_gpu_render.py) and their view"""
    below = float(np.nextafter(np.float32(8.0), np.float32(0.0)))
    rows = [(0.0, 0.0, 1.0, 0.5), (8.0, 1.0, 1.0, 0.5), (below, 1.0, 1.0, 0.5), (-0.0, 2.0, 1.0, 0.5), (3.0, -0.0, 1.0, 0.5),
            (6.0, 2.0, 1.0, 1.0), (2.5, 1.5, 1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0)))), (np.nan, 1.0, 1.0, 0.5),
            (1.0, np.inf, 1.0, 0.5), (2.0, 2.0, 1.0, np.nan), (2.0, 2.0, 1.0, np.inf), (-np.inf, 0.0, 500.0, 0.5), (-40.0, 2.0, 500.0, 42.0),
            (5.0, 3.0, 0.0, 0.5), (-1.0, 1.0, 0.0, 2.0)]
    a = np.zeros((len(rows), 8), dtype=np.float32)
    a[:, 0], a[:, 1], a[:, 6], a[:, 7] = [np.array(c, dtype=np.float32) for c in zip(*rows)]
    return ob.partition(a)[0], rr.make_view((0.0, 0.0), (0.0, 0.0), 1.0, 8, 4, 100.0)
