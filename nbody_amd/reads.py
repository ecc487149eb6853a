"""The read-only calls of a world or an ensemble, written once.

SimPipeline, SimBatch, World and WorldBatch inherit `Reads` and state only what differs between them:

    _lib          the library the entry points live in, resolved at the call: hip_lib or nbody_lib
    _ENTRY        method name -> C entry point, one column of ENTRY_POINTS below
    _WORLD_LAYER  the World layer takes profile / pair_counts / neighbours / groups arguments as a World*Spec structure and fills in a
                  NULL palette itself; the seam (nb_hip_*) takes them loose and wants a palette
    _n            particles per world (total_len at the seam, size in the World layer)
    count         an ensemble's members; None for a single world
    offsets       a ragged ensemble's member boundaries in a packed array; None otherwise

A single world answers with (n, ...) arrays, an ensemble with a leading B; what has one entry per particle (potential,
neighbours) comes from a ragged ensemble as a list of per-member arrays.
"""
import ctypes as C

import numpy as np

from ._abi import (NB_NEIGH_ALL, NB_NEIGH_MASSIVE, NB_NEIGH_MASSLESS, NB_PAIRS_ALL, NB_PAIRS_COLUMNS, NB_PAIRS_MM, NB_PAIRS_MT,
                   NB_PAIRS_TT, NB_PROFILE_BY_MASS, NB_PROFILE_BY_NUMBER, NB_PROFILE_QTY, RenderView, WorldEnergy,
                   WorldGroupSpec, WorldNeighbourSpec, WorldPairSpec, WorldProfileSpec, as_points, default_palette)

# method             SimPipeline                 SimBatch                            World                      WorldBatch
ENTRY_POINTS = {
    "energy":           ("nb_hip_energy",           "nb_hip_ensemble_energy",           "GetWorldEnergy",          "GetWorldBatchEnergy"),
    "potential":        ("nb_hip_potential",        "nb_hip_ensemble_potential",        "GetWorldPotential",       "GetWorldBatchPotential"),
    "potential_at":     ("nb_hip_potential_at",     "nb_hip_ensemble_potential_at",     "GetWorldPotentialAt",     "GetWorldBatchPotentialAt"),
    "potential_map":    ("nb_hip_potential_map",    "nb_hip_ensemble_potential_map",    "RenderWorldPotential",    "RenderWorldBatchPotential"),
    "acceleration_at":  ("nb_hip_acceleration_at",  "nb_hip_ensemble_acceleration_at",  "GetWorldAccelerationAt",  "GetWorldBatchAccelerationAt"),
    "acceleration_map": ("nb_hip_acceleration_map", "nb_hip_ensemble_acceleration_map", "RenderWorldAcceleration", "RenderWorldBatchAcceleration"),
    "tidal_at":         ("nb_hip_tidal_at",         "nb_hip_ensemble_tidal_at",         "GetWorldTidalAt",         "GetWorldBatchTidalAt"),
    "tidal_map":        ("nb_hip_tidal_map",        "nb_hip_ensemble_tidal_map",        "RenderWorldTidal",        "RenderWorldBatchTidal"),
    "profile":          ("nb_hip_profile",          "nb_hip_ensemble_profile",          "GetWorldProfile",         "GetWorldBatchProfile"),
    "pair_counts":      ("nb_hip_pair_counts",      "nb_hip_ensemble_pair_counts",      "GetWorldPairCounts",      "GetWorldBatchPairCounts"),
    "neighbours":       ("nb_hip_neighbours",       "nb_hip_ensemble_neighbours",       "GetWorldNeighbours",      "GetWorldBatchNeighbours"),
    "groups":           ("nb_hip_groups",           "nb_hip_ensemble_groups",           "GetWorldGroups",          "GetWorldBatchGroups"),
    "bounds":           ("nb_hip_bounds",           "nb_hip_ensemble_bounds",           "GetWorldBounds",          "GetWorldBatchBounds"),
    "render_counts":    ("nb_hip_render_counts",    "nb_hip_ensemble_render_counts",    "RenderWorldCounts",       "RenderWorldBatchCounts"),
    "render":           ("nb_hip_render_rgba",      "nb_hip_ensemble_render_rgba",      "RenderWorld",             "RenderWorldBatch"),
}
COLUMNS = ("SimPipeline", "SimBatch", "World", "WorldBatch")


def entry_points(cls):
    """The column of ENTRY_POINTS that is class `cls`: its _ENTRY."""
    return {method: row[COLUMNS.index(cls)] for method, row in ENTRY_POINTS.items()}


def _unpacked(flat, offsets):
    return [flat[int(offsets[b]):int(offsets[b + 1])].copy() for b in range(len(offsets) - 1)]


def _member_points(points, count):
    """(n, 2) points for every member, or (count, n, 2) with one set per member -> contiguous float32 (count, n, 2)."""
    a = np.asarray(points, dtype=np.float32)
    if a.ndim == 2:
        a = np.broadcast_to(a, (count,) + a.shape)
    if a.ndim != 3 or a.shape[0] != count or a.shape[2] != 2:
        raise ValueError(f"points must have shape (n, 2) or ({count}, n, 2)")
    return np.ascontiguousarray(a)


def _profile_args(edges, centre, centre_velocity, weights, count=None):
    """(edges float32 (bins + 1,), bins, centres float32 (4,) or (count, 4) as (cx, cy, ux, uy), weights as the C enum)."""
    e = np.ascontiguousarray(edges, dtype=np.float32)
    if e.ndim != 1 or e.shape[0] < 2:
        raise ValueError("edges must be a sequence of at least two radii")
    modes = {"mass": NB_PROFILE_BY_MASS, "number": NB_PROFILE_BY_NUMBER, NB_PROFILE_BY_MASS: NB_PROFILE_BY_MASS,
             NB_PROFILE_BY_NUMBER: NB_PROFILE_BY_NUMBER}
    if isinstance(weights, (str, int)) and weights in modes:
        mode = modes[weights]
    elif isinstance(weights, (int, np.integer)):
        mode = int(weights)          # the library names the fault
    else:
        raise ValueError('weights must be "mass" or "number"')
    c, u = np.asarray(centre, dtype=np.float32), np.asarray(centre_velocity, dtype=np.float32)
    if count is None:
        if c.shape != (2,) or u.shape != (2,):
            raise ValueError("centre and centre_velocity must have shape (2,)")
        return e, e.shape[0] - 1, np.ascontiguousarray(np.concatenate([c, u])), mode
    for a in (c, u):
        if a.shape != (2,) and a.shape != (count, 2):
            raise ValueError(f"centre and centre_velocity must have shape (2,) or ({count}, 2)")
    both = np.empty((count, 4), dtype=np.float32)
    both[:, 0:2], both[:, 2:4] = c, u
    return e, e.shape[0] - 1, both, mode


def _profile_specs(e, bins, centres, mode):
    """One WorldProfileSpec per row of centres (count, 4), all pointing at the edges e."""
    specs = (WorldProfileSpec * centres.shape[0])()
    for b, row in enumerate(centres):
        specs[b].edges, specs[b].bins, specs[b].weights = e.ctypes.data, bins, mode
        specs[b].centre[0], specs[b].centre[1] = row[0], row[1]
        specs[b].centre_velocity[0], specs[b].centre_velocity[1] = row[2], row[3]
    return specs


def _pair_args(edges, classes):
    """(edges float32 (bins + 1,), bins, classes as the C bit mask)."""
    e = np.ascontiguousarray(edges, dtype=np.float32)
    if e.ndim != 1 or e.shape[0] < 2:
        raise ValueError("edges must be a sequence of at least two radii")
    names = {"mm": NB_PAIRS_MM, "mt": NB_PAIRS_MT, "tt": NB_PAIRS_TT, "all": NB_PAIRS_ALL}
    if isinstance(classes, (int, np.integer)) and not isinstance(classes, bool):
        return e, e.shape[0] - 1, int(classes) & 0xffffffff          # the library names the fault
    if isinstance(classes, str):
        classes = (classes,)
    mask = 0
    try:
        for c in classes:
            mask |= names[c]
    except (KeyError, TypeError):
        raise ValueError('classes must be a subset of "mm", "mt", "tt", or "all"') from None
    if mask == 0:
        raise ValueError('classes must name at least one of "mm", "mt", "tt"')
    return e, e.shape[0] - 1, mask


def _neigh_mask(name, what):
    names = {"massive": NB_NEIGH_MASSIVE, "massless": NB_NEIGH_MASSLESS, "all": NB_NEIGH_ALL}
    if isinstance(name, (int, np.integer)) and not isinstance(name, bool):
        return int(name) & 0xffffffff          # the library names the fault
    try:
        return names[name]
    except (KeyError, TypeError):
        raise ValueError(f'{what} must be "massive", "massless" or "all"') from None


class Reads:
    """What can be asked of a world, or of every member of an ensemble, without changing it.  `views` is one RenderView for a
    single world; for an ensemble one RenderView for all members or a sequence of one per member (width and height are the
    first's).  `points` is (n, 2) for a single world; for an ensemble (n, 2) for all members or (B, n, 2)."""

    _WORLD_LAYER = False
    count = None
    offsets = None

    def _fn(self, method):
        return getattr(self._lib(), self._ENTRY[method])

    def _lead(self):
        """The leading axes of every result: none for a single world, (B,) for an ensemble."""
        return () if self.count is None else (self.count,)

    def _per_particle(self, dtype):
        """An array with one entry per particle: (n,), (B, n), or the packed (sum N_b,) of a ragged ensemble."""
        if self.offsets is not None:
            return np.empty(int(self.offsets[-1]), dtype=dtype)
        return np.empty(self._lead() + (self._n,), dtype=dtype)

    def _members(self, a):
        """A per-particle array as it is returned: a ragged ensemble's as a list of per-member copies."""
        return a if self.offsets is None else _unpacked(a, self.offsets)

    def _views(self, views):
        """(what the library takes for `views`: one RenderView by reference, or RenderView[count]; height; width)."""
        if self.count is None:
            return C.byref(views), views.height, views.width
        if isinstance(views, RenderView):
            views = [views] * self.count
        views = list(views)
        if len(views) != self.count:
            raise ValueError(f"expected one RenderView or {self.count} of them")
        arr = (RenderView * self.count)()
        for b, v in enumerate(views):
            C.memmove(C.byref(arr[b]), C.byref(v), C.sizeof(RenderView))
        return arr, int(arr[0].height), int(arr[0].width)

    def _field_at(self, method, points, softening, *tail):
        pts = as_points(points) if self.count is None else _member_points(points, self.count)
        out = np.empty(pts.shape[:-1] + tail, dtype=np.float32)
        self._fn(method)(self._h, pts.ctypes.data, pts.shape[-2], softening, out.ctypes.data)
        return out

    def _field_map(self, method, views, softening, *tail):
        arg, h, w = self._views(views)
        out = np.empty(self._lead() + (h, w) + tail, dtype=np.float32)
        self._fn(method)(self._h, arg, softening, out.ctypes.data)
        return out

    def energy(self):
        """Kinetic / potential / total energy, mass, momentum, angular momentum, centre of mass (float64; include/nbody_diag.h)
        as a dict (WorldEnergy.as_dict); an ensemble gives a list of one dict per member, each bit-identical to that of the same
        particles alone."""
        out = (WorldEnergy * (1 if self.count is None else self.count))()
        self._fn("energy")(self._h, out)
        return out[0].as_dict() if self.count is None else [e.as_dict() for e in out]

    def potential(self):
        """Phi_i of every particle, float32 (n,) in the order the object keeps its particles (partitioned; particles() /
        member(b) of the World layer); an ensemble (B, n), a ragged one a list of B (N_b,) arrays."""
        out = self._per_particle(np.float32)
        self._fn("potential")(self._h, out.ctypes.data)
        return self._members(out)

    def potential_at(self, points, softening):
        """Phi at the points with one softening (include/nbody_field.h), float32 (n,); an ensemble (B, n), ragged ones
        included, member b's row bit-identical to that of the same particles alone."""
        return self._field_at("potential_at", points, softening)

    def potential_map(self, views, softening):
        """Phi at every pixel centre of the view, float32 (height, width); an ensemble (B, height, width)."""
        return self._field_map("potential_map", views, softening)

    def acceleration_at(self, points, softening):
        """g at the points with one softening (include/nbody_gravity.h), float32 (n, 2); an ensemble (B, n, 2)."""
        return self._field_at("acceleration_at", points, softening, 2)

    def acceleration_map(self, views, softening):
        """g at every pixel centre of the view, float32 (height, width, 2); an ensemble (B, height, width, 2)."""
        return self._field_map("acceleration_map", views, softening, 2)

    def tidal_at(self, points, softening):
        """The tidal tensor dg/dp at the points with one softening (include/nbody_tidal.h), float32 (n, 3) in the order
        (xx, xy, yy); an ensemble (B, n, 3), ragged ones included."""
        return self._field_at("tidal_at", points, softening, 3)

    def tidal_map(self, views, softening):
        """The tidal tensor at every pixel centre of the view, float32 (height, width, 3); an ensemble (B, height, width, 3)."""
        return self._field_map("tidal_map", views, softening, 3)

    def profile(self, edges, centre=(0.0, 0.0), centre_velocity=(0.0, 0.0), weights="mass", return_unplaced=False):
        """The annulus moments about `centre` moving with `centre_velocity` (include/nbody_profile.h), float64 (bins + 2, 6) with
        the columns (count, S, I, L, W, K); row 0 lies inside edges[0], row bins + 1 at or beyond edges[-1].  weights: "mass"
        (massive particles, weight m) or "number" (all particles, weight 1).  With return_unplaced also the number of particles
        whose squared radius is NaN, an int.  A natural centre: energy()["center_of_mass"] and momentum / mass (vel is used as
        stored, the caveat of include/nbody_diag.h).  nb.profile_curves / nb.lagrangian_radii read the result.
        An ensemble, ragged ones included: (B, bins + 2, 6) and uint32 (B,); the edges are shared, centre and centre_velocity
        are (2,) for all members or (B, 2); member b's rows are bit-identical to those of the same particles alone."""
        e, bins, c, mode = _profile_args(edges, centre, centre_velocity, weights, self.count)
        out = np.empty(self._lead() + (bins + 2, NB_PROFILE_QTY), dtype=np.float64)
        lost = np.zeros(1 if self.count is None else self.count, dtype=np.uint32)
        if self._WORLD_LAYER:       # GetWorldProfile(world, spec, ...), GetWorldBatchProfile(batch, specs, count, ...)
            specs = _profile_specs(e, bins, c.reshape(-1, 4), mode)
            self._fn("profile")(self._h, specs, *self._lead(), out.ctypes.data, lost.ctypes.data)
        else:
            self._fn("profile")(self._h, e.ctypes.data, bins, c.ctypes.data, mode, out.ctypes.data, lost.ctypes.data)
        if not return_unplaced:
            return out
        return out, (int(lost[0]) if self.count is None else lost)

    def pair_counts(self, edges, classes=("mm",), return_unplaced=False):
        """The pairs of particles per row of separations and per class (include/nbody_paircount.h), uint64 (bins + 2, 3) with the
        columns (massive-massive, massive-massless, massless-massless); row 0 lies inside edges[0], row bins + 1 at or beyond
        edges[-1].  classes: any subset of "mm", "mt", "tt", or "all"; a class not asked for is zeros and is never evaluated.
        With return_unplaced also the pairs per class whose squared separation is NaN, uint64 (3,).  Every count is exact: device,
        host and numpy agree bit for bit.  nb.profile_edges makes edges, nb.pair_curves reads the result.
        An ensemble, in one launch for all members: (B, bins + 2, 3) and (B, 3)."""
        e, bins, mask = _pair_args(edges, classes)
        out = np.zeros(self._lead() + (bins + 2, NB_PAIRS_COLUMNS), dtype=np.uint64)
        lost = np.zeros(self._lead() + (NB_PAIRS_COLUMNS,), dtype=np.uint64)
        args = (C.byref(WorldPairSpec(e.ctypes.data, bins, mask)),) if self._WORLD_LAYER else (e.ctypes.data, bins, mask)
        self._fn("pair_counts")(self._h, *args, out.ctypes.data, lost.ctypes.data)
        return (out, lost) if return_unplaced else out

    def neighbours(self, radius=None, receivers="all", sources="all"):
        """The nearest neighbour of every particle (include/nbody_neighbour.h): (q, index), or (q, index, count) when a radius is
        given -- q float32, the squared distance to the closest other particle of `sources` (+inf without one); index uint32,
        which one (the smallest index among equal q; nb.NB_NEIGH_NONE without one); count uint32, how many lie within `radius`.
        receivers / sources: "massive", "massless" or "all"; a particle that is no receiver gets (+inf, NONE, 0) and a class that
        is neither is never read.  Device, host and numpy agree bit for bit.  nb.neighbour_distance and nb.closest_pairs read
        the result.  Shapes (N,), in the order potential() has.
        An ensemble, in one launch for all members: (B, N), a ragged one lists of per-member arrays, as potential() gives; an
        index counts within its member."""
        r, s = _neigh_mask(receivers, "receivers"), _neigh_mask(sources, "sources")
        q, index = self._per_particle(np.float32), self._per_particle(np.uint32)
        count = None if radius is None else self._per_particle(np.uint32)
        h = 0.0 if radius is None else float(radius)
        args = (C.byref(WorldNeighbourSpec(r, s, h)),) if self._WORLD_LAYER else (r, s, h)
        self._fn("neighbours")(self._h, *args, q.ctypes.data, index.ctypes.data, None if count is None else count.ctypes.data)
        return tuple(self._members(a) for a in ((q, index) if count is None else (q, index, count)))

    def groups(self, linking_length, members="all", return_count=False):
        """The friends-of-friends groups under `linking_length` (include/nbody_group.h): uint32 labels (N,), in the order
        potential() has -- for every particle the smallest index among the particles it is connected to through any chain of
        pairs closer than the linking length (its own index with none); nb.NB_GROUP_NONE for a particle outside `members`.
        members: "massive", "massless" or "all"; a class that is not of it is never read and bridges nothing.  With return_count
        also the number of groups, an int.  Device, host and numpy agree bit for bit.  nb.group_table and nb.group_members read
        the result, nb.linking_length_for chooses a length.
        An ensemble, in one call for all members: (B, N) and uint32 (B,); a ragged one a list of per-member arrays, as
        neighbours() gives; a label counts within its member, so no group crosses members."""
        mask = _neigh_mask(members, "members")
        labels = self._per_particle(np.uint32)
        found = np.zeros(1 if self.count is None else self.count, dtype=np.uint32)
        length = float(linking_length)
        args = (C.byref(WorldGroupSpec(mask, length)),) if self._WORLD_LAYER else (mask, length)
        self._fn("groups")(self._h, *args, labels.ctypes.data, found.ctypes.data if return_count else None)
        if not return_count:
            return self._members(labels)
        return self._members(labels), (int(found[0]) if self.count is None else found)

    def bounds(self):
        """float32 [min.x, min.y, max.x, max.y] over the particles with finite x and y (include/nbody_render.h); an ensemble
        (B, 4).  Ragged ensembles are not rendered: bounds / render_counts / render end the process there."""
        out = np.empty(self._lead() + (4,), dtype=np.float32)
        self._fn("bounds")(self._h, out.ctypes.data)
        return out

    def render_counts(self, views):
        """The particles of each class covering each pixel, uint32 (3, height, width); an ensemble (B, 3, height, width)."""
        arg, h, w = self._views(views)
        out = np.empty(self._lead() + (3, h, w), dtype=np.uint32)
        self._fn("render_counts")(self._h, arg, out.ctypes.data)
        return out

    def render(self, views, palette=None):
        """The frame, uint8 (height, width, 4); an ensemble (B, height, width, 4).  palette None = DefaultRenderPalette."""
        arg, h, w = self._views(views)
        out = np.empty(self._lead() + (h, w, 4), dtype=np.uint8)
        if palette is None and not self._WORLD_LAYER:
            palette = default_palette()
        self._fn("render")(self._h, arg, None if palette is None else C.byref(palette), out.ctypes.data)
        return out
