"""The definitions of include/nbody_render.h restated in numpy float32 (a plain helper module; no GPU, no library).

Every float32 operation is one numpy operation on float32 arrays, so each is rounded on its own like the C code built with
-ffp-contract=off.  Points go through np.bincount, discs through a loop over the (few) discs near the screen that tests
EVERY pixel of the image -- no bounding box, so a box that is too narrow in the library shows up as a difference; only discs
further than 1 % of their radius plus two pixels from the screen (float64) are skipped -- and the shade is uint32."""
import numpy as np

F = np.float32
MAX_PIXELS = 1 << 24


def make_view(target, offset, zoom, width, height, core_mass):
    import nbody_amd as nb
    return nb.RenderView.make([float(F(t)) for t in target], [float(F(o)) for o in offset], float(F(zoom)), int(width), int(height),
                              float(F(core_mass)))


def view_fields(view):
    return (F(view.target[0]), F(view.target[1]), F(view.offset[0]), F(view.offset[1]), F(view.zoom), int(view.width),
            int(view.height), F(view.core_mass))


def classify(part, view):
    """Per particle: class, sx, sy, rho (float32), and the masks `point` / `disc` (dropped particles are in neither)."""
    tx, ty, ox, oy, zoom, width, height, core = view_fields(view)
    x, y, mass, radius = (np.ascontiguousarray(part[:, c], dtype=F) for c in (0, 1, 6, 7))
    with np.errstate(all="ignore"):
        sx = (x - tx) * zoom + ox
        sy = (y - ty) * zoom + oy
        rho = radius * zoom
    cls = np.where(mass <= F(0), 0, np.where(mass < core, 1, 2)).astype(np.int64)
    keep = np.isfinite(sx) & np.isfinite(sy) & np.isfinite(rho)
    disc = keep & (rho >= F(1))
    point = keep & ~disc
    return {"cls": cls, "sx": sx, "sy": sy, "rho": rho, "point": point, "disc": disc}


def points_in_view(c, view):
    width, height = int(view.width), int(view.height)
    sx, sy = c["sx"], c["sy"]
    with np.errstate(invalid="ignore"):
        return c["point"] & (sx >= F(0)) & (sx < F(width)) & (sy >= F(0)) & (sy < F(height))


def disc_cover(sx, sy, rho, width, height):
    """bool (height, width): the pixels one disc covers."""
    px = np.arange(width, dtype=np.uint32).astype(F)
    py = np.arange(height, dtype=np.uint32).astype(F)
    with np.errstate(over="ignore"):
        dx = (px + F(0.5)) - F(sx)
        dy = (py + F(0.5)) - F(sy)
        xx, yy = dx * dx, dy * dy
        d2 = yy[:, None] + xx[None, :]          # float32 addition commutes: xx + yy
        r2 = F(rho) * F(rho)
    return d2 <= r2


def describe(part, view):
    """What a view holds, from this module's own classification: points in view per class, and per disc its class,
    covered pixels and whether its centre is on screen."""
    c = classify(part, view)
    width, height = int(view.width), int(view.height)
    inview = points_in_view(c, view)
    discs = []
    for i in np.flatnonzero(c["disc"]):
        sx, sy, rho = c["sx"][i], c["sy"][i], c["rho"][i]
        reach = float(rho) * 1.01 + 2.0
        if float(sx) + reach < 0 or float(sx) - reach > width or float(sy) + reach < 0 or float(sy) - reach > height:
            covered = 0     # far off screen (checked generously in float64); the full test below would say the same
        else:
            covered = int(np.count_nonzero(disc_cover(sx, sy, rho, width, height)))
        centre_on = bool(0 <= float(sx) < width and 0 <= float(sy) < height)
        discs.append({"index": int(i), "cls": int(c["cls"][i]), "covered": covered, "centre_on_screen": centre_on})
    return {"points": [int(np.count_nonzero(inview & (c["cls"] == k))) for k in range(3)],
            "discs": discs, "discs_on_screen": sum(1 for d in discs if d["covered"] > 0)}


def counts(part, view):
    """uint32 (3, height, width)."""
    width, height = int(view.width), int(view.height)
    assert width >= 1 and height >= 1 and width * height <= MAX_PIXELS
    c = classify(part, view)
    plane = width * height
    inview = points_in_view(c, view)
    px = c["sx"][inview].astype(np.uint32).astype(np.int64)
    py = c["sy"][inview].astype(np.uint32).astype(np.int64)
    word = c["cls"][inview] * plane + py * width + px
    out = np.bincount(word, minlength=3 * plane).astype(np.uint32).reshape(3, height, width)
    for i in np.flatnonzero(c["disc"]):
        sx, sy, rho = c["sx"][i], c["sy"][i], c["rho"][i]
        reach = float(rho) * 1.01 + 2.0
        if float(sx) + reach < 0 or float(sx) - reach > width or float(sy) + reach < 0 or float(sy) - reach > height:
            continue
        out[c["cls"][i]] += disc_cover(sx, sy, rho, width, height).astype(np.uint32)
    return out


def shade(cnt, background, color, saturation):
    """uint8 (height, width, 4) from uint32 (3, height, width); all arithmetic uint32 (wrapping)."""
    cnt = cnt.astype(np.uint32)
    sat = np.uint32(saturation)
    bg = np.asarray(background, dtype=np.uint32)
    col = np.asarray(color, dtype=np.uint32)
    cls = np.where(cnt[2] > 0, 2, np.where(cnt[1] > 0, 1, np.where(cnt[0] > 0, 0, -1)))
    n = np.where(cls == 2, cnt[2], np.where(cls == 1, cnt[1], cnt[0])).astype(np.uint32)
    t = np.minimum(n, sat).astype(np.uint32)
    out = np.empty(cnt.shape[1:] + (4,), dtype=np.uint8)
    with np.errstate(over="ignore"):
        for ch in range(4):
            c = col[np.maximum(cls, 0), ch].astype(np.uint32)
            v = (bg[ch] * (sat - t) + c * t + sat // np.uint32(2)) // sat
            out[..., ch] = np.where(cls >= 0, v, bg[ch]).astype(np.uint32) & np.uint32(0xff)
    return out


def shade_with(cnt, palette):
    return shade(cnt, list(palette.background), [list(c) for c in palette.color], int(palette.saturation))


def order_key(v):
    u = np.ascontiguousarray(v, dtype=F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def bounds(part):
    """float32 [min.x, min.y, max.x, max.y] over the particles with finite x and y, floats in their total order."""
    x, y = np.ascontiguousarray(part[:, 0], dtype=F), np.ascontiguousarray(part[:, 1], dtype=F)
    ok = np.isfinite(x) & np.isfinite(y)
    if not ok.any():
        return np.array([np.inf, np.inf, -np.inf, -np.inf], dtype=F)
    x, y = x[ok], y[ok]
    kx, ky = order_key(x), order_key(y)
    return np.array([x[np.argmin(kx)], y[np.argmin(ky)], x[np.argmax(kx)], y[np.argmax(ky)]], dtype=F)


def min_gc_mass():
    """MIN_GC_MASS of include/galaxy.h in float32: (4 * PI * 30 / 3) * 200 * 200 * 200, left to right."""
    pi, dens, r = F(3.1415927), F(30.0), F(200.0)
    return F(F(F(F(F(4.0) * pi) * dens) / F(3.0)) * r * r * r)


def fit_view_fields(b, width, height):
    """(target, offset, zoom) of FitWorldView from bounds b, in float32."""
    w, h = F(width), F(height)
    offset = (w * F(0.5), h * F(0.5))
    if b[0] > b[2]:
        return (F(0), F(0)), offset, F(1)
    target = (F(0.5) * (b[0] + b[2]), F(0.5) * (b[1] + b[3]))
    ex, ey = b[2] - b[0], b[3] - b[1]
    with np.errstate(all="ignore"):
        if ex > 0 and ey > 0:
            zoom = F(0.9) * min(w / ex, h / ey)
        elif ex > 0:
            zoom = F(0.9) * (w / ex)
        elif ey > 0:
            zoom = F(0.9) * (h / ey)
        else:
            zoom = F(1)
    return target, offset, F(zoom)


def fit_view(part, width, height):
    target, offset, zoom = fit_view_fields(bounds(part), width, height)
    return make_view(target, offset, zoom, width, height, min_gc_mass())


# ---- the views the render tests share (built from this module's own numbers, never from the library under test) ------

def heaviest(part):
    return int(np.argmax(part[:, 6]))


def edge_view(part, width=1280, height=720):
    """zoom 8z; the heaviest particle's centre lies half its on-screen radius to the LEFT of the left edge."""
    fit = fit_view(part, width, height)
    c = heaviest(part)
    zoom = F(8) * F(fit.zoom)
    rho = float(F(part[c, 7]) * zoom)
    ox, oy = width * 0.5, height * 0.5
    tx = float(part[c, 0]) + (ox + 0.5 * rho) / float(zoom)
    return make_view((tx, float(part[c, 1])), (ox, oy), zoom, width, height, min_gc_mass())


def mixed_view(part, width=1280, height=720):
    """zoom 0.25 centred on the ordinary massive particle nearest the heaviest one."""
    c = heaviest(part)
    core = min_gc_mass()
    ordinary = np.flatnonzero((part[:, 6] > 0) & (part[:, 6] < core))
    d = np.hypot(part[ordinary, 0].astype(np.float64) - float(part[c, 0]), part[ordinary, 1].astype(np.float64) - float(part[c, 1]))
    o = int(ordinary[np.argmin(d)])
    return make_view((part[o, 0], part[o, 1]), (width * 0.5, height * 0.5), 0.25, width, height, core)


def collapsed_view(part, width=1280, height=720):
    """the fitted zoom / 4096: every particle lands in the pixel at the middle of the screen."""
    fit = fit_view(part, width, height)
    return make_view((fit.target[0], fit.target[1]), (width // 2 + 0.5, height // 2 + 0.5), F(fit.zoom) / F(4096), width, height,
                     min_gc_mass())


def empty_view(part, width=1280, height=720):
    """the fitted zoom, looking ten extents to the right of everything."""
    fit = fit_view(part, width, height)
    b = bounds(part)
    return make_view((float(b[2]) + 10.0 * float(b[2] - b[0]) + 1.0e4, fit.target[1]), (width * 0.5, height * 0.5), fit.zoom, width,
                     height, min_gc_mass())


def check_mix(part, view, want_points=False, want_discs=False, want_off_centre_disc=False):
    """Asserts, from this module's classification, that a view holds what it was chosen for; returns the description."""
    d = describe(part, view)
    if want_points:
        assert sum(d["points"]) > 0, d["points"]
    if want_discs:
        assert d["discs_on_screen"] > 0
    if want_off_centre_disc:
        off = [x for x in d["discs"] if x["covered"] > 0 and not x["centre_on_screen"]]
        assert len(off) >= 1, "no disc with an off-screen centre covers a pixel"
    return d
