"""Rendering a WorldBatch (include/nbody_batch_render.h) without a GPU: the exported surface, the host path member by member
BITWISE against the numpy restatement (tests/render_ref.py), the limits, and nb.contact_sheet.  A WorldBatch that never
stepped answers on the host, so nothing here opens a device.

Views per member come from batch_render_common.make_view (render_ref's views; a member without an ordinary massive particle
is shown through its fitted view in the "mixed" set, see there)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
import render_ref as rr
from batch_render_common import CUSTOM, KINDS, hand_made, make_view
from gpu_common import synth

ROOT = nb.ROOT
SIZES = [(64, 48), (37, 53)]


def members_333(golden, count):
    """ic_333, a member with no massive particle and one with only massive ones (333 particles each)."""
    return np.stack([golden("ic_333.bin"), synth(333, 0.0, seed=1)[0], synth(333, 1.0, seed=2)[0]][:count])


def check_batch(wb, views, palette=None):
    """bounds, counts and frames of every member against numpy; returns the count images."""
    parts = [wb.member(b) for b in range(wb.count)]
    bounds, cnt, img = wb.bounds(), wb.render_counts(views), wb.render(views, palette)
    pal = palette if palette is not None else nb.default_palette()
    per_member = [views] * wb.count if isinstance(views, nb.RenderView) else views
    assert bounds.shape == (wb.count, 4) and bounds.dtype == np.float32
    assert cnt.shape == (wb.count, 3, per_member[0].height, per_member[0].width) and cnt.dtype == np.uint32
    assert img.shape == (wb.count, per_member[0].height, per_member[0].width, 4) and img.dtype == np.uint8
    for b, part in enumerate(parts):
        want = rr.counts(part, per_member[b])
        assert bounds[b].tobytes() == rr.bounds(part).tobytes(), b
        assert np.array_equal(cnt[b], want), (b, int(np.count_nonzero(cnt[b] != want)))
        assert np.array_equal(img[b], rr.shade_with(want, pal)), b
    return cnt


def test_the_library_exports_the_new_surface_and_the_hooks_stay_out_of_the_public_headers():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_batch_render.h")).read(), flags=re.S)
    names = re.findall(r"^\s*void\s+(\w+)\s*\(", text, re.M)
    assert set(names) == {"GetWorldBatchBounds", "FitWorldBatchViews", "RenderWorldBatchCounts", "RenderWorldBatch"}
    nm = lambda so: subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout.split()  # noqa: E731
    assert set(names) <= set(nm(nb.NBODY_SO)) and set(names) <= set(nb.NBODY_API)
    seam = {"nb_hip_ensemble_bounds", "nb_hip_ensemble_render_counts", "nb_hip_ensemble_render_rgba"}
    hooks = {"nb_hip_ensemble_render_mode", "nb_hip_ensemble_last_render_info", "nb_hip_ensemble_last_render_ms"}
    have = set(nm(nb.HIP_SO))
    assert seam | hooks <= have and seam <= set(nb.HIP_API) and hooks <= set(nb.TUNE_API)
    public = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    tuning = open(os.path.join(ROOT, "nbody_amd", "csrc", "nbody_hip_tuning.h")).read()
    for name in hooks:
        assert re.search(r"\b%s\s*\(" % name, tuning) and name not in public and name not in text, name
    for name in seam:
        assert re.search(r"\b%s\s*\(" % name, public), name
    assert "WorldBatch is not covered" not in open(os.path.join(ROOT, "include", "nbody_render.h")).read()
    make = open(os.path.join(ROOT, "nbody_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\brender_kernels\b", make, re.M)


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("width,height", SIZES)
def test_host_path_against_the_numpy_restatement(golden, count, width, height):
    wb = nb.WorldBatch(members_333(golden, count))
    parts = [wb.member(b) for b in range(count)]
    fitted = wb.fit_views(width, height)
    for b, part in enumerate(parts):
        assert bytes(fitted[b]) == bytes(rr.fit_view(part, width, height)), b
    custom = nb.RenderPalette.make(**CUSTOM)
    for kind in KINDS:
        views = [make_view(kind, part, width, height) for part in parts]
        cnt = check_batch(wb, views)
        check_batch(wb, views, custom)
        # member 0 is ic_333: the views hold what they were chosen for
        d = rr.check_mix(parts[0], views[0], want_points=kind == "fitted", want_discs=kind == "mixed",
                         want_off_centre_disc=kind == "edge")
        if kind == "mixed" and count == 3:      # the all-massive member holds ordinary massive particles: its discs are drawn too
            rr.check_mix(parts[2], views[2], want_points=False, want_discs=True, want_off_centre_disc=False)
        if kind == "collapsed":
            assert all(int(cnt[b][:, height // 2, width // 2].sum()) == 333 == int(cnt[b].sum()) for b in range(count))
        if kind == "nothing":
            assert not cnt.any() and d["discs_on_screen"] == 0
    # every member in its own view kind, in one call
    check_batch(wb, [make_view(KINDS[b % len(KINDS)], part, width, height) for b, part in enumerate(parts)])
    assert wb.particles().tobytes() == np.stack(parts).tobytes()
    wb.close()


def test_a_single_view_is_broadcast(golden):
    wb = nb.WorldBatch(members_333(golden, 3))
    view = rr.mixed_view(wb.member(0), 64, 48)
    cnt = check_batch(wb, view)
    assert np.array_equal(cnt, wb.render_counts([view] * 3)) and np.array_equal(wb.render(view), wb.render([view, view, view]))
    with pytest.raises(ValueError):
        wb.render_counts([view, view])
    wb.close()


def test_hand_made_edges_and_non_finite_particles_as_one_member_among_ordinary_ones():
    hand, view = hand_made()
    n = hand.shape[0]
    nothing_finite = np.full((n, 8), np.nan, dtype=np.float32)
    wb = nb.WorldBatch(np.stack([synth(n, 0.5, seed=3, extent=3.0)[0], hand, synth(n, 1.0, seed=4, extent=3.0)[0], nothing_finite]))
    cnt = check_batch(wb, view)
    assert cnt[1][0].any() and cnt[1][1].any() and cnt[1][2].any()       # a massless disc, points and an off-screen core disc
    assert wb.bounds()[3].tolist() == [np.inf, np.inf, -np.inf, -np.inf] and not cnt[3].any()
    fitted = wb.fit_views(8, 4)
    assert (fitted[3].zoom, fitted[3].target[0], fitted[3].target[1]) == (1.0, 0.0, 0.0)
    check_batch(wb, fitted)
    wb.close()


CHILD = ("import ctypes as C, numpy as np, nbody_amd as nb\n"
         "a = np.zeros((3, 4, 8), dtype=np.float32); a[:, :, 0] = np.arange(4); a[:, :, 6] = 1; a[:, :, 7] = 0.25\n"
         "wb = nb.WorldBatch(a); L = nb.nbody_lib()\n"
         "def views(w=(4, 4, 4), h=4, zoom=1.0):\n"
         "    return (nb.RenderView * 3)(*[nb.RenderView.make((0.0, 0.0), (0.0, 0.0), zoom, w[b], h, 1.0) for b in range(3)])\n"
         "out = np.zeros(3 * 3 * 64, dtype=np.uint32)\n"
         "pal = nb.default_palette()\n")
ABORTS = [("differing width", "L.RenderWorldBatchCounts(wb._h, views(w=(4, 4, 5)), out.ctypes.data)", r"member 2 of 3.*differ from member 0"),
          ("too many pixels", "L.RenderWorldBatchCounts(wb._h, views(w=(4096,) * 3, h=2048), out.ctypes.data)",
           r"count \* width \* height must not exceed 2\^24"),
          ("zero zoom", "L.RenderWorldBatch(wb._h, views(zoom=0.0), None, out.ctypes.data)", r"member 0 of 3.*zoom must be finite and > 0"),
          ("zero saturation", "pal.saturation = 0; L.RenderWorldBatch(wb._h, views(), C.byref(pal), out.ctypes.data)",
           r"saturation must be at least 1"),
          ("NULL counts", "L.RenderWorldBatchCounts(wb._h, views(), None)", r"NULL argument"),
          ("NULL frames", "L.RenderWorldBatch(wb._h, views(), None, None)", r"NULL argument"),
          ("NULL bounds", "L.GetWorldBatchBounds(wb._h, None)", r"NULL argument"),
          ("SimBatch before set_data", "s = nb.SimBatch(4, [4, 4, 4]); nb.hip_lib().nb_hip_ensemble_render_counts(s._h, views(), out.ctypes.data)",
           r"nb_hip_ensemble_render_counts before nb_hip_batch_set_data"),
          ("SimBatch bounds before set_data", "s = nb.SimBatch(4, [4, 4, 4]); nb.hip_lib().nb_hip_ensemble_bounds(s._h, out.ctypes.data)",
           r"nb_hip_ensemble_bounds before nb_hip_batch_set_data")]


@pytest.mark.parametrize("name,call,needle", ABORTS, ids=[a[0] for a in ABORTS])
def test_a_violation_prints_file_line_func_and_aborts(name, call, needle):
    r = subprocess.run([sys.executable, "-c", CHILD + call + "\nprint('SURVIVED')\n"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(c|hip):\d+ \[\w+\]", r.stderr) and re.search(needle, r.stderr), r.stderr


def test_a_world_batch_that_never_stepped_renders_without_opening_a_device():
    code = ("import os, numpy as np, nbody_amd as nb\n"
            "a = np.zeros((3, 64, 8), dtype=np.float32); a[:, :, 0] = np.arange(64); a[:, :, 6] = 1; a[:, :, 7] = 0.25\n"
            "wb = nb.WorldBatch(a); v = wb.fit_views(64, 16); c = wb.render_counts(v); f = wb.render(v); b = wb.bounds(); wb.close()\n"
            "fds = []\n"
            "for f_ in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f_))\n"
            "    except OSError: pass\n"
            "assert not [x for x in fds if x == '/dev/kfd' or x.startswith('/dev/dri/')], fds\n"
            "print('OK', int(c.sum()), f.shape, b.shape)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK 192 (3, 16, 64, 4) (3, 4)"


def test_contact_sheet_shapes_and_placement():
    frames = np.arange(5 * 2 * 3 * 4, dtype=np.uint8).reshape(5, 2, 3, 4) + 1
    sheet = nb.contact_sheet(frames, 2)
    assert sheet.shape == (3 * 2, 2 * 3, 4) and sheet.dtype == np.uint8
    for b in range(5):
        r, c = divmod(b, 2)
        assert np.array_equal(sheet[r * 2:(r + 1) * 2, c * 3:(c + 1) * 3], frames[b]), b
    assert not sheet[4:6, 3:6].any()                                       # the missing sixth cell
    assert nb.contact_sheet(frames, 5).shape == (2, 15, 4) and nb.contact_sheet(frames, 7).shape == (2, 21, 4)
    assert np.array_equal(nb.contact_sheet(frames, 1), frames.reshape(10, 3, 4))
    with pytest.raises(ValueError):
        nb.contact_sheet(frames, 0)
