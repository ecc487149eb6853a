"""The return conventions of the read-only methods on the seam: the table of tests/test_binding_surface_cpu.py, the same worlds
(N = 5 with 3 massive: both classes of particle, all three classes of pair; a ragged ensemble of 5 and 1) and the same arguments,
on SimPipeline, SimBatch and SimBatch.ragged -- and every member of the SimBatch bit for bit the SimPipeline of its particles.
Each call launches a few workgroups."""
import numpy as np
import pytest

import nbody_amd as nb
import test_binding_surface_cpu as surface

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def massive(a):
    return int(np.count_nonzero(a[:, 6] > 0))


def pipeline(a):
    p = nb.SimPipeline(a.shape[0], massive(a))
    p.set_data(a)
    return p


def batch(states):
    b = nb.SimBatch(states.shape[1], [massive(a) for a in states])
    b.set_data(states)
    return b


def ragged(members):
    b = nb.SimBatch.ragged([a.shape[0] for a in members], [massive(a) for a in members])
    b.set_data(members)
    return b


def test_what_every_read_returns_on_the_device():
    surface.surface_of(pipeline, batch, ragged)
