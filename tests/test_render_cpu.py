"""Rendering (include/nbody_render.h) without a GPU: the host path of GetWorldBounds / FitWorldView / RenderWorldCounts /
RenderWorld against the numpy restatement of the definitions (tests/render_ref.py), BITWISE; the header / binding / export
agreement; and static checks on the ISA of nbody_amd/csrc/render_kernels.hip (the kernels of a world and of an ensemble)."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import nbody_amd as nb
import render_ref as rr
from isa_common import compile_isa, functions, kernel_meta

ROOT = nb.ROOT
RENDER_FUNCS = {"DefaultRenderPalette", "GetWorldBounds", "FitWorldView", "RenderWorldCounts", "RenderWorld"}
HIP_FUNCS = {"nb_hip_bounds", "nb_hip_render_counts", "nb_hip_render_rgba"}
WORLDS = ["ic_333", "ic_1024", "ic_4096", "galaxies_65536"]


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", text, re.M)


def exported(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


_cache = {}


def world_particles(name, golden):
    """The World's partitioned particles of a named world (CPU only)."""
    if name not in _cache:
        ic = nb.make_galaxies(65536, 2, seed=11037) if name == "galaxies_65536" else golden(name + ".bin")
        w = nb.World(ic)
        _cache[name] = w.particles()
        w.close()
    return _cache[name]


def host_render(part, view, palette=None):
    """(counts, frame, particles before, particles after) of a CPU-only World of these particles."""
    w = nb.World(part)
    before = w.particles()
    cnt = w.render_counts(view)
    img = w.render(view, palette)
    after = w.particles()
    w.close()
    return cnt, img, before, after


def check_view(part, view, palette=None):
    cnt, img, before, after = host_render(part, view, palette)
    want = rr.counts(part, view)
    assert cnt.dtype == np.uint32 and cnt.shape == (3, view.height, view.width)
    assert np.array_equal(cnt, want), f"{np.count_nonzero(cnt != want)} words differ"
    assert img.dtype == np.uint8 and img.shape == (view.height, view.width, 4)
    assert np.array_equal(img, rr.shade_with(want, palette if palette is not None else nb.default_palette()))
    assert before.tobytes() == after.tobytes()          # particles() is byte-identical before and after every call
    return cnt


# ---- the surface ----------------------------------------------------------------------------------------------------------

def test_render_header_binding_and_exports_agree():
    assert set(declared_functions("nbody_render.h")) == RENDER_FUNCS
    assert RENDER_FUNCS <= set(nb.NBODY_API) and RENDER_FUNCS <= exported(nb.NBODY_SO)
    assert HIP_FUNCS <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and HIP_FUNCS <= exported(nb.HIP_SO)
    assert "nb_hip_last_render_ms" in nb.TUNE_API and "nb_hip_last_render_ms" in exported(nb.HIP_SO)
    assert not {"nb_cpu_bounds", "nb_cpu_render_counts", "nb_cpu_render_rgba", "nb_fit_view"} & exported(nb.NBODY_SO)
    assert nb.hip_lib().nb_hip_version() == 400      # no version bump: the new surface is detected by its symbols
    for h in ("nbody.h", "galaxy.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not [f for f in RENDER_FUNCS if f in text]


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_render_header_compiles_as_c11_and_cxx_with_the_bound_layout(compiler, std, ext):
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "nbody_render.h"\n'
           'int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(RenderView), offsetof(RenderView, offset), '
           'offsetof(RenderView, zoom), offsetof(RenderView, width), offsetof(RenderView, height), offsetof(RenderView, core_mass), '
           'sizeof(RenderPalette), offsetof(RenderPalette, color), offsetof(RenderPalette, saturation)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t." + ext), "w").write(src)
        subprocess.run([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t." + ext), "-o", os.path.join(d, "t")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.split()]
    V, P = nb.RenderView, nb.RenderPalette
    assert out == [C.sizeof(V), V.offset.offset, V.zoom.offset, V.width.offset, V.height.offset, V.core_mass.offset,
                   C.sizeof(P), P.color.offset, P.saturation.offset]


# ---- host path = render_ref, bitwise ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", WORLDS)
def test_fitted_view(golden, name):
    part = world_particles(name, golden)
    w = nb.World(part)
    view = w.fit_view(1280, 720)
    assert np.array_equal(w.bounds(), rr.bounds(part)) and w.bounds().tobytes() == rr.bounds(part).tobytes()
    w.close()
    assert bytes(view) == bytes(rr.fit_view(part, 1280, 720))
    # the three fixtures show their two cores as discs of a few pixels; the 65 536-particle galaxy pair is so wide that even
    # its cores are points on a fitted 1280 x 720 screen
    d = rr.check_mix(part, view, want_points=True, want_discs=name.startswith("ic_"))
    print(f"[render] {name} fitted: points {d['points']}, discs on screen {[(x['cls'], x['covered']) for x in d['discs'] if x['covered']]}")
    cnt = check_view(part, view)
    # every finite particle is on the fitted screen: each class's sum = its points + its discs' covered pixels
    for k in range(3):
        assert int(cnt[k].sum(dtype=np.uint64)) == d["points"][k] + sum(x["covered"] for x in d["discs"] if x["cls"] == k)
    assert sum(d["points"]) + len(d["discs"]) == part.shape[0]


@pytest.mark.parametrize("name", WORLDS)
def test_edge_view_a_disc_centred_off_screen_still_covers_pixels(golden, name):
    part = world_particles(name, golden)
    view = rr.edge_view(part)
    d = rr.check_mix(part, view, want_points=True, want_off_centre_disc=True)
    off = [x for x in d["discs"] if x["covered"] > 0 and not x["centre_on_screen"]]
    print(f"[render] {name} edge: points {d['points']}, off-centre discs {[(x['cls'], x['covered']) for x in off]}")
    assert any(x["index"] == rr.heaviest(part) for x in off)
    cnt = check_view(part, view)
    for k in range(3):
        assert int(cnt[k].sum(dtype=np.uint64)) == d["points"][k] + sum(x["covered"] for x in d["discs"] if x["cls"] == k)


@pytest.mark.parametrize("name", WORLDS)
def test_mixed_view_discs_beside_points(golden, name):
    part = world_particles(name, golden)
    view = rr.mixed_view(part)
    d = rr.check_mix(part, view, want_points=True, want_discs=True)
    print(f"[render] {name} mixed: points {d['points']}, discs on screen {d['discs_on_screen']}")
    assert d["discs_on_screen"] >= 2
    cnt = check_view(part, view)
    for k in range(3):
        assert int(cnt[k].sum(dtype=np.uint64)) == d["points"][k] + sum(x["covered"] for x in d["discs"] if x["cls"] == k)


@pytest.mark.parametrize("name", WORLDS)
def test_collapsed_view_holds_every_particle_in_one_pixel(golden, name):
    part = world_particles(name, golden)
    view = rr.collapsed_view(part)
    cnt = check_view(part, view)
    core = rr.min_gc_mass()
    per_class = [int(np.count_nonzero(part[:, 6] <= 0)), int(np.count_nonzero((part[:, 6] > 0) & (part[:, 6] < core))),
                 int(np.count_nonzero(part[:, 6] >= core))]
    assert sum(per_class) == part.shape[0]
    assert [int(v) for v in cnt[:, 360, 640]] == per_class
    assert int(cnt.sum(dtype=np.uint64)) == part.shape[0]


@pytest.mark.parametrize("name", WORLDS)
def test_a_view_that_sees_nothing_one_pixel_and_an_odd_size(golden, name):
    part = world_particles(name, golden)
    cnt = check_view(part, rr.empty_view(part))
    assert not cnt.any()
    one = rr.fit_view(part, 1, 1)
    assert check_view(part, one).shape == (3, 1, 1)
    odd = rr.fit_view(part, 37, 53)
    d = rr.check_mix(part, odd, want_points=True)
    assert int(check_view(part, odd).sum(dtype=np.uint64)) >= sum(d["points"])
    big_disc = rr.make_view((part[rr.heaviest(part), 0], part[rr.heaviest(part), 1]), (18.5, 26.5), 1.0, 37, 53, rr.min_gc_mass())
    assert check_view(part, big_disc)[2].all()       # the core's disc (radius >= 200 px) fills the 37 x 53 screen


# ---- edge semantics on hand-made particles ------------------------------------------------------------------------------------

def particle(x, y, mass=1.0, radius=0.5):
    return [x, y, 0.0, 0.0, 0.0, 0.0, mass, radius]


UNIT = dict(target=(0.0, 0.0), offset=(0.0, 0.0), zoom=1.0, core_mass=100.0)


def unit_view(width=8, height=4, **kw):
    f = dict(UNIT, **kw)
    return rr.make_view(f["target"], f["offset"], f["zoom"], width, height, f["core_mass"])


def test_points_at_the_screen_edges():
    below = float(np.nextafter(np.float32(8.0), np.float32(0.0)))
    a = np.array([particle(0.0, 0.0), particle(8.0, 1.0), particle(below, 1.0), particle(-0.0, 2.0), particle(3.0, -0.0),
                  particle(float(np.nextafter(np.float32(0.0), np.float32(-1.0))), 3.0), particle(2.5, 4.0), particle(7.999, 3.999)],
                 dtype=np.float32)
    view = unit_view()
    cnt = check_view(a, view)
    want = np.zeros((4, 8), dtype=np.uint32)
    for x, y in ((0, 0), (7, 1), (0, 2), (3, 0), (7, 3)):      # exactly 0, just below width, -0 in x, -0 in y, the far corner
        want[y, x] += 1
    assert np.array_equal(cnt[1], want) and not cnt[0].any() and not cnt[2].any()     # x = width, y = height, x < 0: nowhere


def test_non_finite_particles_are_dropped_and_do_not_disturb_the_bounds():
    good = [particle(1.5, 1.5), particle(-3.0, 2.0, mass=0.0), particle(6.0, -1.0, mass=500.0)]
    bad = [particle(np.nan, 1.0), particle(1.0, np.nan), particle(np.inf, 1.0), particle(1.0, -np.inf), particle(-np.inf, np.inf),
           particle(2.0, 2.0, radius=np.nan), particle(2.0, 2.0, radius=np.inf), particle(2.0, 2.0, radius=-np.inf)]
    a = np.array(good + bad, dtype=np.float32)
    w = nb.World(a)
    part = w.particles()
    b = w.bounds()
    w.close()
    # radius does not enter the bounds: the three particles with a non-finite radius at (2, 2) are inside them anyway
    assert b.tolist() == [-3.0, -1.0, 6.0, 2.0] and b.tobytes() == rr.bounds(part).tobytes()
    cnt = check_view(part, unit_view(offset=(0.0, 1.0)))
    assert int(cnt.sum(dtype=np.uint64)) == 2 and cnt[1, 2, 1] == 1 and cnt[2, 0, 6] == 1
    # signed zeros and the total order: -0 sorts below +0 whatever the particle order
    z = np.array([particle(0.0, -0.0), particle(-0.0, 0.0)], dtype=np.float32)
    for arr in (z, z[::-1]):
        w = nb.World(arr)
        got = w.bounds()
        w.close()
        assert got.tobytes() == np.array([-0.0, -0.0, 0.0, 0.0], dtype=np.float32).tobytes() == rr.bounds(arr).tobytes()


def test_rho_just_below_one_is_a_point_and_exactly_one_is_a_disc():
    below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    a = np.array([particle(2.5, 1.5, radius=below), particle(6.0, 2.0, radius=1.0)], dtype=np.float32)
    cnt = check_view(a, unit_view())[1]
    assert cnt[1, 2] == 1 and int(cnt[:, :4].sum()) == 1           # a point: its own pixel only, although it is centred in it
    # the disc of radius exactly 1 centred on the pixel corner (6, 2): the four pixels around it (dx^2 + dy^2 = 0.5 <= 1)
    assert int(cnt[:, 4:].sum()) == 4 and cnt[1, 5] == cnt[1, 6] == cnt[2, 5] == cnt[2, 6] == 1
    c = rr.classify(a, unit_view())
    assert c["point"].tolist() == [True, False] and c["disc"].tolist() == [False, True]


# ---- invariants ---------------------------------------------------------------------------------------------------------------

def test_shuffling_the_callers_particles_changes_nothing(golden):
    ic = golden("ic_1024.bin")
    part = world_particles("ic_1024", golden)
    rng = np.random.default_rng(5)
    for view in (rr.fit_view(part, 1280, 720), rr.mixed_view(part), rr.collapsed_view(part)):
        base = host_render(ic, view)[:2]
        for _ in range(2):
            got = host_render(ic[rng.permutation(ic.shape[0])], view)[:2]
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


def test_host_result_does_not_depend_on_the_thread_count():
    code = ("import sys, hashlib, numpy as np, nbody_amd as nb\n"
            "sys.path.insert(0, 'tests')\n"
            "import render_ref as rr\n"
            "ic = np.fromfile('tests/golden/ic_4096.bin', dtype=np.float32).reshape(-1, 8)\n"
            "w = nb.World(ic); p = w.particles(); h = hashlib.sha256()\n"
            "for v in (w.fit_view(640, 360), rr.mixed_view(p, 640, 360), rr.collapsed_view(p, 640, 360)):\n"
            "    h.update(w.render_counts(v).tobytes()); h.update(w.render(v).tobytes())\n"
            "h.update(w.bounds().tobytes()); sys.stdout.write(h.hexdigest())\n")
    outs = []
    for threads in ("1", "4"):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, OMP_NUM_THREADS=threads), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1] and len(outs[0]) == 64


def test_cpu_only_world_renders_without_opening_a_device():
    code = ("import os, numpy as np, nbody_amd as nb\n"
            "a = np.zeros((64, 8), dtype=np.float32); a[:, 0] = np.arange(64); a[:, 6] = 1; a[:, 7] = 0.25\n"
            "w = nb.World(a); w.update_cpu(0.01, 2); v = w.fit_view(64, 16); c = w.render_counts(v); f = w.render(v); w.close()\n"
            "fds = []\n"
            "for f_ in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f_))\n"
            "    except OSError: pass\n"
            "assert not [x for x in fds if x == '/dev/kfd' or x.startswith('/dev/dri/')], fds\n"
            "print('OK', int(c.sum()), f.shape)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK 64 (16, 64, 4)"


# ---- shade ----------------------------------------------------------------------------------------------------------------------

def test_shade_is_the_integer_formula():
    # one row of pixels with hand-made counts, through particles: k massless points in pixel k, and priority cases
    rows = []
    for k in range(1, 7):
        rows += [particle(k + 0.5, 0.5, mass=0.0)] * k
    rows += [particle(0.5, 1.5, mass=0.0)] * 3 + [particle(0.5, 1.5, mass=1.0)]                                  # ordinary beats massless
    rows += [particle(1.5, 1.5, mass=0.0)] * 2 + [particle(1.5, 1.5, mass=1.0)] * 5 + [particle(1.5, 1.5, mass=200.0, radius=0.1)]
    a = np.array(rows, dtype=np.float32)
    view = unit_view(width=8, height=2)
    for sat in (1, 4, 5, 255, 1000):
        pal = nb.RenderPalette.make((10, 20, 30, 40), ((200, 100, 0, 255), (1, 2, 3, 4), (255, 254, 253, 128)), sat)
        cnt = check_view(a, view, pal)
        img = host_render(a, view, pal)[1]
        assert cnt[0, 0, 1:7].tolist() == [1, 2, 3, 4, 5, 6] and cnt[:, 1, 0].tolist() == [3, 1, 0] and cnt[:, 1, 1].tolist() == [2, 5, 1]
        assert img[0, 0].tolist() == [10, 20, 30, 40] and img[0, 7].tolist() == [10, 20, 30, 40]           # background, alpha carried
        for k in range(1, 7):
            t = min(k, sat)
            assert img[0, k].tolist() == [(b * (sat - t) + c * t + sat // 2) // sat for b, c in zip((10, 20, 30, 40), (200, 100, 0, 255))]
        t = min(1, sat)
        assert img[1, 0].tolist() == [(b * (sat - t) + c * t + sat // 2) // sat for b, c in zip((10, 20, 30, 40), (1, 2, 3, 4))]
        assert img[1, 1].tolist() == [(b * (sat - t) + c * t + sat // 2) // sat for b, c in zip((10, 20, 30, 40), (255, 254, 253, 128))]
        if sat <= 4:
            assert img[0, 4].tolist() == img[0, 6].tolist() == [200, 100, 0, 255]                        # a count above saturation
    d = nb.default_palette()
    assert d.saturation >= 1 and list(d.background) != list(d.color[2])


# ---- FitWorldView and the limits --------------------------------------------------------------------------------------------------

def test_fit_view_formula_zero_extent_and_empty():
    a = np.array([particle(-100.0, 10.0), particle(300.0, 50.0, mass=0.0)], dtype=np.float32)
    w = nb.World(a)
    v = w.fit_view(1280, 720)
    w.close()
    assert (v.zoom, v.target[0], v.target[1], v.offset[0], v.offset[1]) == (float(np.float32(0.9) * np.float32(3.2)), 100.0, 30.0, 640.0, 360.0)
    assert np.float32(v.core_mass) == rr.min_gc_mass() and bytes(v) == bytes(rr.fit_view(a, 1280, 720))
    # a vertical line: x does not constrain; a single point and an empty World: zoom 1
    for arr, zoom, target in ((np.array([particle(5.0, 0.0), particle(5.0, 90.0)], dtype=np.float32), float(np.float32(0.9) * np.float32(8.0)), (5.0, 45.0)),
                              (np.array([particle(0.0, 7.0), particle(64.0, 7.0)], dtype=np.float32), float(np.float32(0.9) * np.float32(20.0)), (32.0, 7.0)),
                              (np.array([particle(3.0, 4.0)], dtype=np.float32), 1.0, (3.0, 4.0)),
                              (np.array([particle(np.nan, 4.0)], dtype=np.float32), 1.0, (0.0, 0.0)),
                              (np.zeros((0, 8), dtype=np.float32), 1.0, (0.0, 0.0))):
        w = nb.World(arr)
        v = w.fit_view(1280, 720)
        assert (v.zoom, v.target[0], v.target[1]) == (zoom, *target) and bytes(v) == bytes(rr.fit_view(arr, 1280, 720)), arr
        cnt, img = w.render_counts(v), w.render(v)
        w.close()
        assert np.array_equal(cnt, rr.counts(arr, v))
        if arr.shape[0] == 0 or not np.isfinite(arr[:, 0]).all():
            assert not cnt.any() and np.array_equal(img, np.broadcast_to(np.array(list(nb.default_palette().background), dtype=np.uint8), img.shape))
    assert rr.bounds(np.zeros((0, 8), dtype=np.float32)).tolist() == [np.inf, np.inf, -np.inf, -np.inf]


BAD_VIEWS = [("zero width", "0, 4, 1.0", "width and height must be at least 1"),
             ("zero height", "4, 0, 1.0", "width and height must be at least 1"),
             ("too many pixels", "4097, 4096, 1.0", "must not exceed 2^24"),
             ("zero zoom", "4, 4, 0.0", "zoom must be finite and > 0"),
             ("negative zoom", "4, 4, -1.0", "zoom must be finite and > 0"),
             ("nan zoom", "4, 4, float('nan')", "zoom must be finite and > 0"),
             ("infinite zoom", "4, 4, float('inf')", "zoom must be finite and > 0")]


@pytest.mark.parametrize("name,args,needle", BAD_VIEWS, ids=[b[0] for b in BAD_VIEWS])
def test_an_invalid_view_prints_file_line_func_and_aborts(name, args, needle):
    code = ("import numpy as np, nbody_amd as nb\n"
            "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
            "w = nb.World(a)\n"
            f"width, height, zoom = {args}\n"
            "v = nb.RenderView.make((0.0, 0.0), (0.0, 0.0), zoom, width, height, 1.0)\n"
            "out = np.zeros((3, max(height, 1), max(min(width, 8), 1)), dtype=np.uint32)\n"
            "nb.nbody_lib().RenderWorldCounts(w._h, v, out.ctypes.data)\nprint('SURVIVED')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.c:\d+ \[\w+\]", r.stderr) and needle in r.stderr, r.stderr


def test_a_sharded_world_aborts_with_the_diagnostics_message():
    code = ("import nbody_amd as nb, numpy as np, ctypes as C\n"
            "a = np.zeros((16, 8), dtype=np.float32); a[:, 0] = np.arange(16); a[:, 6] = 1; a[:, 7] = 1\n"
            "L = nb.nbody_lib(); fn = nb.ALLGATHER_FN(lambda *x: None)\n"
            "w = L.CreateWorldShardedWith(a.ctypes.data, 16, 0, 2, fn, None)\n"
            "b = np.zeros(4, dtype=np.float32); L.GetWorldBounds(w, b.ctypes.data); print('SURVIVED')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout
    assert re.search(r"\.c:\d+ \[\w+\]", r.stderr) and "sharded pipeline needs a collective" in r.stderr, r.stderr


# ---- static ISA of render_kernels.hip -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def render_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("render_isa"), "render_kernels.hip")


def test_render_kernels_exist_without_scratch_and_add_with_native_integer_atomics(render_isa):
    make = open(os.path.join(ROOT, "nbody_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\brender\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*render_cpu\.c", make, re.M)
    assert re.search(r"^HIP_TUS\s*:=.*\brender_kernels\b", make, re.M)
    meta = kernel_meta(render_isa)
    for kernel in ("bounds_kernel", "splat_kernel", "disc_kernel", "shade_kernel", "ensemble_bounds_kernel", "ensemble_splat_kernel",
                   "ensemble_tile_kernel", "ensemble_disc_kernel", "ensemble_shade_kernel"):
        rows = [m for m in meta if kernel in m[0]]
        assert rows and all(m[0].startswith("_ZN2nb") for m in rows), (kernel, [m[0] for m in meta])
        for name, scratch, sgpr, vgpr in rows:
            print(f"[render isa] {name}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs")
            assert scratch == 0 and vgpr <= 64, (name, scratch, vgpr)     # 64 VGPRs: eight waves per SIMD
    # a world's splat: the shipped merge and the one-atomic-per-lane A/B build; the tile kernel: counts and frames; the disc pass
    # and the shade: one plain kernel for a world, one for an ensemble (DESIGN.md "Rendering an ensemble" says why not one for both)
    instances = {k: len([m for m in meta if re.search(r"\d%s(I|E)" % k, m[0])])
                 for k in ("splat_kernel", "ensemble_splat_kernel", "ensemble_tile_kernel", "disc_kernel", "shade_kernel",
                           "ensemble_disc_kernel", "ensemble_shade_kernel")}
    assert instances == {"splat_kernel": 2, "ensemble_splat_kernel": 1, "ensemble_tile_kernel": 2, "disc_kernel": 1, "shade_kernel": 1,
                         "ensemble_disc_kernel": 1, "ensemble_shade_kernel": 1}, instances
    body = functions(render_isa)
    ops = {k: [i.split()[0] for i in v] for k, v in body.items()}
    # the 32-bit unsigned integer add: gfx950 (like every gfx9) spells it global_atomic_add; gfx11+ assemblers print the same
    # instruction as global_atomic_add_u32.  Either spelling, and never a float form or a compare-and-swap loop.
    add = re.compile(r"^global_atomic_add(_u32)?$")
    for kernel in ("splat_kernel", "disc_kernel"):
        for name in [n for n in ops if kernel in n]:
            assert any(add.match(o) for o in ops[name]), name
    every = [o for v in ops.values() for o in v]
    assert not [o for o in every if "cmpswap" in o or "atomic_add_f" in o or "atomic_pk" in o or o.startswith("scratch_")]
    # every atomic on device memory is a global_ one, never flat_ or buffer_ (the tile kernel's LDS adds are ds_ operations)
    assert not [o for o in every if "atomic" in o and not o.startswith("global_atomic_")]
    # no-return adds (no sc0) on the count image; the only returning add is the disc list's cursor
    merged = next(n for n in body if "splat_kernel" in n and "Lb1" in n)
    for name in [n for n in body if "splat_kernel" in n]:   # a world's two and the ensemble's
        adds = [i for i in body[name] if add.match(i.split()[0])]
        assert [i for i in adds if "sc0" not in i] and any("sc0" in i for i in adds), name
    assert all("sc0" not in i for n in body if "disc_kernel" in n for i in body[n] if add.match(i.split()[0]))
    # the merge: a broadcast of the first live lane's word and a population count of the ballot
    assert "v_readlane_b32" in ops[merged] and any(o.startswith("s_bcnt1_i32_b64") for o in ops[merged])
