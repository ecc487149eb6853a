"""The one wall-clock assertion of the renderer: looking at a resident world must cost less than reading it back.

N = 2^20 bench workload (srand(11037), 2 galaxies), fitted 1280 x 720 view, one pipeline, one process, after a warm-up
call each, interleaved, fastest of 5 wall-clock times each: a blocking render() (clear + splat + disc + shade + 3.7 MB to
the host) must take LESS than a blocking get_data() of the same pipeline (merge kernel + 32 MiB to the host), the cheapest
first half of the only route to a picture there was before.  No further margin is fixed."""
import time

import pytest

import nbody_amd as nb
import render_ref as rr
from gpu_common import bench_universe

pytestmark = pytest.mark.gpu


def test_render_beats_reading_the_particles_back():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    _, part, m = bench_universe(1 << 20)
    view = rr.fit_view(part, 1280, 720)
    sim = nb.SimPipeline(part.shape[0], m)
    sim.set_data(part)
    sim.update(1, 0.01)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    wall(lambda: sim.render(view)), wall(sim.get_data)          # warm-up call each
    r, g = [], []
    for _ in range(5):
        r.append(wall(lambda: sim.render(view)))
        g.append(wall(sim.get_data))
    device_ms = sim.last_render_ms()[0]
    sim.close()
    print(f"[render] N=2^20 fitted 1280x720: render {min(r):.3f} ms wall ({device_ms:.3f} ms on the device), get_data {min(g):.3f} ms wall, "
          f"ratio {min(g) / min(r):.1f}x")
    assert min(r) < min(g), (r, g)
