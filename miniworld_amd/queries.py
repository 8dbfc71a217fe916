"""The world queries of the batched env — navigation fields, explored-area maps, grid sight, grid regions, grid clearance, egocentric map windows,
depth projection, label frames, object maps, ray casts, scan maps, scan evidence, scan matching, scan weighing and resampling, grid rollouts —, each one kernel on the device with no host value: their value
classes (NavField, SeenMap, EgoWindow, DepthWindow, DepthMap, LabelFrame, ObjectWindow, ObjectMap, GridRegions, GridClearance, ScanMap, ScanEvidence, ScanMatch, ScanWeights, GridRollout) and
`WorldQueries`, a mixin of MiniWorldVecEnv (vec_env.py)."""
from __future__ import annotations

import math

import numpy as np

from . import engine as eng
from ._args import integer, real


class NavField:
    """A navigation field (MiniWorldVecEnv.nav_field): `field`, the uint16[N, gz, gx] device tensor of shortest-path costs — 0xFFFF a
    blocked cell, 0xFFFE one no path reaches, a move costs 5 straight and 7 diagonally —, the grid (`cell` metres per cell, gx x gz
    cells from the env's own min_x, min_z), and what it leads to: `target`, an entity slot or a float64[N, 3] device tensor.  The
    tensor is the caller's, like a level bank: the engine keeps nothing of it.  A field of grid_field() — built over the caller's own
    maps — has `obstacles` "grid", `target` None or the tensor of points, and `margin` is its whole inflation radius."""

    def __init__(self, field, params, target, obstacles):
        self.field, self.params, self.target, self.obstacles = field, params, target, obstacles

    cell = property(lambda self: self.params.cell)
    margin = property(lambda self: self.params.margin)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)

    @property
    def points(self):
        """the device tensor of point targets, or None for a slot target"""
        return None if isinstance(self.target, int) else self.target


class SeenMap:
    """An explored-area map (MiniWorldVecEnv.seen_map): `seen`, the uint8[N, gz, gx] device tensor — 1 where the env's agent has had
    the cell's centre in sight since the row was last cleared —, `count`, int32[N], the cells seen so far, `new`, int32[N], those the
    last seen_update() added, and the grid (`cell` metres per cell, gx x gz cells from the env's own min_x, min_z: a nav field's).
    `max_range` (metres), `cos_half` (cos(fov / 2); -1: all round) and `obstacles` say what sight is.  The tensors are the caller's,
    like a nav field's: the engine keeps nothing of them, and a fork indexes them with its own `src`."""

    def __init__(self, seen, count, new, params, max_range, cos_half, obstacles):
        self.seen, self.count, self.new, self.params = seen, count, new, params
        self.max_range, self.cos_half, self.obstacles = max_range, cos_half, obstacles

    cell = property(lambda self: self.params.cell)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)


class EgoWindow:
    """An egocentric map window (MiniWorldVecEnv.ego_window): `planes`, the uint8[N, P, S, S] device tensor that ego_update() fills —
    row 0 the farthest ahead, columns growing to the agent's right, points `cell` metres apart —, `names`, its planes in order out of
    ("wall", "entity", "visible"), and the views `wall` (1 in a wall or outside the extent), `entity` (1 + the slot of the entity
    there, 0 for none) and `visible` (1 where the agent sees the point now), each uint8[N, S, S] or None when not asked for.  `back`
    is the anchor in cells behind the window's centre, `frame` "heading" or "north"; `wall_radius`, `entity_pad`, `max_range`,
    `cos_half` and `obstacles` say what the planes mean.  The tensor is the caller's: the engine keeps nothing of it."""
    PLANES = {"wall": eng.EGO_WALL, "entity": eng.EGO_ENTITY, "visible": eng.EGO_VISIBLE}

    def __init__(self, planes, names, size, cell, back, frame, wall_radius, entity_pad, max_range, cos_half, obstacles):
        self.planes, self.names, self.size, self.cell, self.back, self.frame = planes, tuple(names), size, cell, back, frame
        self.wall_radius, self.entity_pad, self.max_range, self.cos_half, self.obstacles = wall_radius, entity_pad, max_range, cos_half, obstacles

    bits = property(lambda self: sum(self.PLANES[n] for n in self.names))

    def _plane(self, name):
        return self.planes[:, self.names.index(name)] if name in self.names else None

    wall = property(lambda self: self._plane("wall"))
    entity = property(lambda self: self._plane("entity"))
    visible = property(lambda self: self._plane("visible"))


class DepthWindow:
    """A depth-projected egocentric window (MiniWorldVecEnv.depth_window): `planes`, the uint8[N, 2, S, S] device tensor that
    depth_update() fills, laid out cell for cell like an EgoWindow of the same size, cell, anchor and frame — row 0 the farthest ahead,
    columns growing to the agent's right —, and its views `floor` (how many pixels of the depth map showed floor in the cell, at most
    255) and `obstacle` (how many showed something between `floor_tol` and `top` above the floor), each uint8[N, S, S].  `min_range`
    and `max_range` bound the eye depth of the pixels that count.  The tensor is the caller's: the engine keeps nothing of it."""

    def __init__(self, planes, size, cell, back, frame, min_range, max_range, floor_tol, top):
        self.planes, self.size, self.cell, self.back, self.frame = planes, size, cell, back, frame
        self.min_range, self.max_range, self.floor_tol, self.top = min_range, max_range, floor_tol, top

    floor = property(lambda self: self.planes[:, 0])
    obstacle = property(lambda self: self.planes[:, 1])


class DepthMap:
    """A depth-built floor-plan map (MiniWorldVecEnv.depth_map): `map`, the uint8[N, 2, gz, gx] device tensor that depth_map_update()
    accumulates on a nav field's grid (`params`: `cell` metres per cell, gx x gz cells from the env's own min_x, min_z), with the views
    `free` (1 once `min_points` pixels of one depth map showed floor in the cell) and `obstacle` (the same for points between `floor_tol`
    and `top` above the floor) — a cell may be both, or neither: never seen —, `count`, int32[N, 2], the cells set so far in each, and
    `new`, int32[N, 2], those the last update added.  The tensors are the caller's, like a SeenMap's."""

    def __init__(self, map, count, new, params, min_points, min_range, max_range, floor_tol, top):
        self.map, self.count, self.new, self.params, self.min_points = map, count, new, params, min_points
        self.min_range, self.max_range, self.floor_tol, self.top = min_range, max_range, floor_tol, top

    cell = property(lambda self: self.params.cell)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)
    free = property(lambda self: self.map[:, 0])
    obstacle = property(lambda self: self.map[:, 1])


class ScanMap:
    """A scan-built floor-plan map (MiniWorldVecEnv.scan_map): `map`, the uint8[N, 2, gz, gx] device tensor that scan_map_update()
    accumulates on a nav field's grid (`params`: `cell` metres per cell, gx x gz cells from the env's own min_x, min_z), laid out like a
    DepthMap's, with the views `free` (1 once a beam passed through the cell) and `obstacle` (1 once a beam that hit something ended in
    it) — a cell may be both over several calls, or neither: never scanned —, `count`, int32[N, 2], the cells set so far in each, and
    `new`, int32[N, 2], those the last update added.  `rays`, `fov`, `max_range` and `obstacles` are the lidar() scan_map_update() casts
    when it is given none; `max_range` also cuts a given scan's beams.  The tensors are the caller's, like a SeenMap's."""

    def __init__(self, map, count, new, params, rays, fov, max_range, obstacles):
        self.map, self.count, self.new, self.params = map, count, new, params
        self.rays, self.fov, self.max_range, self.obstacles = rays, fov, max_range, obstacles

    cell = property(lambda self: self.params.cell)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)
    free = property(lambda self: self.map[:, 0])
    obstacle = property(lambda self: self.map[:, 1])


class ScanEvidence:
    """A scan-built evidence map (MiniWorldVecEnv.scan_evidence): `ev`, the int8[N, gz, gx] device tensor that scan_evidence_update()
    accumulates on a ScanMap's grid (`params`) — up by `hit` per beam that ends in a cell, down by `miss` per beam that passes through
    it, at most `cap` beams a scan, clamped to `lo` .. `hi` —, and what each update rewrites from it: `map`, uint8[N, 2, gz, gx], laid out
    as a ScanMap's with the views `free` (ev <= `free_at`) and `obstacle` (ev >= `occ_at`) — a cell is never both —, `score`,
    uint8[N, gz, gx] = max(ev, 0), a `score` of scan_match(), scan_search() and scan_weigh() as it stands, `count`, int32[N, 2], the
    cells of each plane, and `changed`, int32[N, 2], those the last update moved into or out of each.  `rule` is the seven integers in the
    call's order; `rays`, `fov`, `max_range` and `obstacles` are a ScanMap's.  The tensors are the caller's."""

    def __init__(self, ev, map, score, count, changed, params, rays, fov, max_range, obstacles, rule):
        self.ev, self.map, self.score, self.count, self.changed, self.params = ev, map, score, count, changed, params
        self.rays, self.fov, self.max_range, self.obstacles, self.rule = rays, fov, max_range, obstacles, tuple(rule)
        self.hit, self.miss, self.cap, self.lo, self.hi, self.free_at, self.occ_at = self.rule

    cell = property(lambda self: self.params.cell)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)
    free = property(lambda self: self.map[:, 0])
    obstacle = property(lambda self: self.map[:, 1])


class ScanMatch:
    """Where a scan fits a map (MiniWorldVecEnv.scan_match): `best`, int32[N, 3], the best candidate's (rotation index, a, b) — a whole
    cells along x (columns), b along z (rows) —, `score`, int32[N], its score, and `volume`, int32[N, K, 2 W + 1, 2 W + 1] indexed
    [rotation, b + W, a + W], every candidate's score (None when not asked for).  `angles`, float64[K] on the device, are the rotations in
    radians, centre first: 0, +d, -d, +2d, ...; `rot`, float64[K, 2], their (cos, sin) as the kernel got them; `window` is W, `params` the
    grid, `max_range` the cut.  The tensors are the caller's."""

    def __init__(self, best, score, volume, angles, rot, pairs, window, params, max_range):
        self.best, self.score, self.volume, self.angles, self.rot = best, score, volume, angles, rot
        self.pairs, self.window, self.params, self.max_range = pairs, window, params, max_range     # (pairs: rot's values on the host)

    cell = property(lambda self: self.params.cell)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)

    def offset(self):
        """float64[N, 3]: the correction (a * cell, b * cell, the best rotation's angle) in metres and radians — added to a pose estimate's
        (x, z, dir) —, a new tensor made on the device"""
        import torch
        k = self.best[:, 0].long()
        return torch.stack([self.best[:, 1].double() * self.cell, self.best[:, 2].double() * self.cell, self.angles[k]], 1)

    def apply(self, scan, origin):
        """(scan', origin'): the scan's directions turned by the best rotation — with the kernel's own (cos, sin) — and the origin
        (float64[N, 3]) shifted by the best translation, new tensors made on the device, so that scan_map_update(m, scan', origin') is
        the next line of a mapping loop.  `t` is shared, not copied."""
        import torch
        cs, d = self.rot[self.best[:, 0].long()], scan["dir"]
        c, s = cs[:, None, 0], cs[:, None, 1]
        turned = torch.stack([c * d[..., 0] + s * d[..., 1], c * d[..., 1] - s * d[..., 0]], -1).contiguous()
        moved = origin.clone()
        moved[:, 0] += self.best[:, 1].double() * self.cell
        moved[:, 2] += self.best[:, 2].double() * self.cell
        return dict(scan, dir=turned), moved


class ScanWeights:
    """How well a scan fits a map from each of P poses (MiniWorldVecEnv.scan_weigh): `score`, int32[N, P], the sum of the likelihood bytes
    under the end cells of the scan placed at each particle; `inside`, int32[N, P], how many of its beams ended in the grid; `best`,
    int32[N, 2], the (particle, score) of the highest score, the lowest particle on ties; `pose`, float64[N, P, 4], the rows (x, z, cos,
    sin) exactly as the kernel got them.  `params` is the grid, `max_range` the cut.  The tensors are the caller's."""

    def __init__(self, score, inside, best, pose, params, max_range):
        self.score, self.inside, self.best, self.pose, self.params, self.max_range = score, inside, best, pose, params, max_range

    cell = property(lambda self: self.params.cell)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)


class LabelFrame:
    """A label frame (MiniWorldVecEnv.label_frame): what every pixel of `vec.obs` shows, as label_update() casts it.  `cls`, uint8[N, H, W]:
    0 nothing (sky), 1 floor, 2 ceiling, 3 wall, 4 a static frame (ImageFrame, TextFrame), 5 a Box, 6 a mesh object (engine.LABEL_*);
    `code`, int32[N, H, W]: the static polygon's index, engine.RAY_ENT + slot for an entity, -1 for nothing; `slot`, a view computed
    from it: the entity slot, -1 off entities; `depth`, float32[N, H, W]: the eye depth in metres, `far` for nothing — vec.depth without
    its 16-bit steps, and depth_update(w, depth=f.depth) takes it; `ent_pixels`, int32[N, E]: the pixels that show each slot;
    `ent_box`, int32[N, E, 4]: their box u0, v0, u1, v1 inclusive, (W, H, -1, -1) for a slot out of view.  The tensors not asked for are
    None.  `meshes` ("exact": a mesh object's own triangles; "bounds": its bounding cylinder), `near` and `far` say what was cast.
    The tensors are the caller's: the engine keeps nothing of them."""

    def __init__(self, cls, code, depth, ent_pixels, ent_box, meshes, near, far):
        self.cls, self.code, self.depth, self.ent_pixels, self.ent_box = cls, code, depth, ent_pixels, ent_box
        self.meshes, self.near, self.far = meshes, near, far

    @property
    def slot(self):
        """int32[N, H, W]: the entity slot each pixel shows, -1 off entities (a new tensor); None without `code`"""
        if self.code is None:
            return None
        return (self.code - eng.RAY_ENT).masked_fill_(self.code < eng.RAY_ENT, -1)


class ObjectWindow:
    """A sensed object window (MiniWorldVecEnv.object_window): `plane`, the uint8[N, S, S] device tensor that object_update() fills, laid
    out cell for cell like an EgoWindow's `entity` plane and like a DepthWindow of the same size, cell, anchor and frame: 1 + the id of
    the object whose labelled pixels fell into the cell — the lowest id where several did —, 0 for none.  `min_range`, `max_range`,
    `floor_tol` and `top` say which pixels count, exactly as for a DepthWindow.  The tensor is the caller's: the engine keeps nothing of it."""

    def __init__(self, plane, size, cell, back, frame, min_range, max_range, floor_tol, top):
        self.plane, self.size, self.cell, self.back, self.frame = plane, size, cell, back, frame
        self.min_range, self.max_range, self.floor_tol, self.top = min_range, max_range, floor_tol, top


class ObjectMap:
    """A sensed object map (MiniWorldVecEnv.object_map): `map`, the uint8[N, gz, gx] device tensor that object_map_update() keeps on a nav
    field's grid (`params`: `cell` metres per cell, gx x gz cells from the env's own min_x, min_z) — 1 + the id of the object last seen in
    the cell, 0 for none or never seen; the last observation wins: a cell seen empty forgets its object, a cell out of view keeps it —,
    `cells`, int32[N, ids], how many cells of the map hold each id, and `pos`, float64[N, ids, 3], their centroid (x, 0, z), NaN where
    there are none: `pos[:, q].contiguous()` is a target of grid_field() and nav_field() and a `pos` of nav_query().  The tensors are
    the caller's, like a DepthMap's."""

    def __init__(self, map, cells, pos, params, ids, min_range, max_range, floor_tol, top):
        self.map, self.cells, self.pos, self.params, self.ids = map, cells, pos, params, ids
        self.min_range, self.max_range, self.floor_tol, self.top = min_range, max_range, floor_tol, top

    cell = property(lambda self: self.params.cell)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)


class GridRegions:
    """The connected regions of a byte mask (MiniWorldVecEnv.grid_regions), K = max_regions listed per env in the order of their lowest
    cells: `count`, int32[N], the regions of at least min_cells cells — above K when the list is cut —, `size`, int32[N, K], their cells (0
    for none), `cell`, int32[N, K], each one's representative as a flat index j * gx + i (-1 for none) — a cell of the region itself, and
    a row of it is a `cells` of grid_sight() as it stands —, `sum`, int32[N, K, 2], the sums of its cells' rows and columns, and `label`,
    int16[N, gz, gx]: 0 off the mask, k + 1 in the k-th listed region, -1 in a region that is not listed.  `sum` and `label` are None
    when not asked for.  `params` is the grid; `connectivity` and `min_cells` say what a region is.  The tensors are the caller's."""

    def __init__(self, count, size, cell, sum, label, params, connectivity, min_cells):
        self.count, self.size, self.cell, self.sum, self.label, self.params = count, size, cell, sum, label, params
        self.connectivity, self.min_cells = connectivity, min_cells

    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)
    max_regions = property(lambda self: int(self.size.shape[1]))

    @property
    def centroid(self):
        """float64[N, K, 2]: each listed region's centroid (row, column) in cells, sum / size, NaN for none (a new tensor, made on the
        device); None without `sum`"""
        if self.sum is None:
            return None
        size = self.size.double().unsqueeze(-1)
        return (self.sum.double() / size).masked_fill_(size == 0, float("nan"))


class GridClearance:
    """Every cell's distance to the nearest marked cell of a byte mask (MiniWorldVecEnv.grid_clearance): `dist2`, int32[N, gz, gx], the
    squared distance in cells — 0 on a marked cell, engine.CLEAR_NONE throughout an env without one, engine.CLEAR_FAR beyond the limit —,
    `nearest`, int32[N, gz, gx], that marked cell's flat index j * gx + i, the lowest at a tie, -1 at a sentinel, and `cost`,
    uint8[N, gz, gx], the cost of the first of `bands` — (threshold, cost) integer pairs, thresholds ascending — whose threshold is at
    least dist2, 0 with none: a row of it is an `extra` of grid_field() as it stands.  `nearest` and `cost` are None when not asked for.
    `params` is the grid, `limit` the limit in cells (0: none).  The tensors are the caller's."""

    def __init__(self, dist2, nearest, cost, params, bands, limit):
        self.dist2, self.nearest, self.cost, self.params, self.bands, self.limit = dist2, nearest, cost, params, bands, limit

    cell = property(lambda self: self.params.cell)
    gx = property(lambda self: self.params.gx)
    gz = property(lambda self: self.params.gz)

    def metres(self):
        """float64[N, gz, gx]: sqrt(dist2) * cell, inf at the sentinels (a new tensor, made on the device)"""
        return (self.dist2.double().sqrt() * self.cell).masked_fill_(self.dist2 >= eng.CLEAR_FAR, math.inf)

    @staticmethod
    def threshold(r, cell=0.25):
        """the largest integer t with sqrt(float64(t)) * cell < r, -1 if there is none: grid_field's inflation test, strict and in
        float64, so that (dist2 == 0) | (dist2 <= threshold(r)) are the cells grid_field(inflate=r) blocks.  At most 2^30, which is
        above every dist2 of a grid."""
        r, cell = real("GridClearance.threshold", "r", r, lo_open=False), real("GridClearance.threshold", "cell", cell)
        inside = lambda t: math.sqrt(float(t)) * cell < r
        t = int(min(r / cell, 32768.0) ** 2)        # (clamped first: the square of a huge ratio is no float)
        while t >= 0 and not inside(t):
            t -= 1
        while t < 2 ** 30 and inside(t + 1):
            t += 1
        return t


class GridRollout:
    """What candidate plans would do on the caller's own map (MiniWorldVecEnv.grid_rollout): `pose`, float64[N, P, 3], the final
    (x, z, dir) of each plan; `stats`, int32[N, P, 5], whose columns are the views `reach` — the least field value the plan's poses
    met, the start's included, 0xFFFF without a field —, `reach_step` — the number of steps after which it was first met —, `steps` —
    the steps executed: T unless stop_at ended the plan —, `bumps` — the moves the map refused — and `cost` — the sum of `extra` over
    the poses behind every executed step —; and `trace`, float64[T, N, P, 3], the pose behind every step, or None.  `params` is the
    grid.  The tensors are the caller's."""

    def __init__(self, pose, stats, trace, params):
        self.pose, self.stats, self.trace, self.params = pose, stats, trace, params

    reach = property(lambda self: self.stats[..., 0])
    reach_step = property(lambda self: self.stats[..., 1])
    steps = property(lambda self: self.stats[..., 2])
    bumps = property(lambda self: self.stats[..., 3])
    cost = property(lambda self: self.stats[..., 4])


assert eng.SIGHT_MAX_VIEWS == eng.REGION_MAX        # (a row of GridRegions.cell is a row of grid_sight's cells)
assert eng.NAV_ENTITIES == eng.RAY_ENTITIES == eng.SEEN_ENTITIES == eng.EGO_ENTITIES      # (one table serves the four calls)


class WorldQueries:
    OBSTACLES = {"walls": 0, "walls+entities": eng.NAV_ENTITIES}

    def _obstacle_flags(self, where, obstacles):
        """the engine's flag bits of an `obstacles` name"""
        if obstacles not in self.OBSTACLES:
            raise ValueError(f"{where}: obstacles {obstacles!r}; have {sorted(self.OBSTACLES)}")
        return self.OBSTACLES[obstacles]

    def _grid(self, where, cell):
        """(cell, gx, gz): the grid of `cell` metres per cell over the template world's extent, which the family's constructor arguments fix"""
        cell, t = real(where, "cell", cell), self.template
        gx = max(1, math.ceil((float(t.max_x) - float(t.min_x)) / cell))
        gz = max(1, math.ceil((float(t.max_z) - float(t.min_z)) / cell))
        if gx * gz > eng.NAV_MAX_CELLS:
            raise ValueError(f"{where}: {gx} x {gz} cells > {eng.NAV_MAX_CELLS}: use a larger cell")
        return cell, gx, gz

    def _map_grid(self, where, cell, like, kinds, own):
        """the bare grid (MwNavParams: no margin, reach, flags or target) of a map: `like`'s — one of `kinds`; `own` is how the message
        names its grid — or _grid()'s for `cell`"""
        if like is not None:
            if not isinstance(like, kinds):
                raise ValueError(f"{where}: `like` must be {' or '.join('a ' + k.__name__ for k in kinds)}")
            if cell != 0.25:
                raise ValueError(f"{where}: with `like` {own} grid is used: pass no cell")
            cell, gx, gz = like.params.cell, like.gx, like.gz       # (a GridRegions' `cell` is its representatives)
        else:
            cell, gx, gz = self._grid(where, cell)
        return eng.MwNavParams(float(cell), 0.0, 0.0, int(gx), int(gz), 0, 0)

    def _window_shape(self, where, size, cell, anchor, frame):
        """(size, cell, back, frame) of an egocentric window, checked; `back` is the anchor in cells behind the window's centre"""
        size = integer(where, "size", size, 1, eng.EGO_MAX_SIZE)
        cell = real(where, "cell", cell)
        if anchor not in ("centre", "bottom"):
            raise ValueError(f"{where}: anchor {anchor!r}; have 'centre' and 'bottom'")
        if frame not in ("heading", "north"):
            raise ValueError(f"{where}: frame {frame!r}; have 'heading' and 'north'")
        return size, cell, size / 2 if anchor == "bottom" else 0.0, frame

    def _cos_half(self, where, fov):
        """cos(fov / 2) of a horizontal opening angle in radians, checked; None: default_fov(); 2 pi: -1.0, all round"""
        fov = self.default_fov() if fov is None else real(where, "fov", fov, hi=2 * math.pi)
        return -1.0 if fov == 2 * math.pi else float(math.cos(fov / 2))

    def nav_field(self, target=None, mask=None, cell=0.25, obstacles="walls", margin=None, reach=None, into=None):
        """The shortest-path cost to a target from every cell of a grid over each env's floor plan, walls in the way, built on the
        device by one kernel (mw_nav_build) with no host value and no synchronisation: a NavField.

        target     None: the env's goal entity (cfg.goal_ent); an int: that entity slot — the field starts from the cells where the
                   env's own near() test would hold —; or a float64[N, 3] device tensor of points with `reach` metres around them
        cell       metres per cell; gx, gz follow from the template world's extent, which the family's constructor arguments fix
        obstacles  "walls", or "walls+entities": every listed entity but the target and the carried one blocks cells too
        margin     kept from walls beyond the agent's radius; default cell / 2
        mask       uint8[N] or bool[N] device tensor: only those envs' rows are built (the others are not touched)
        into       a NavField of this call's parameters to rebuild in place — `nav_field(into=field, mask=done)` behind a step keeps
                   the field current across auto-resets; without it a new tensor is allocated (unmasked rows: 0xFFFF)
        An env whose extent the grid does not cover, or one whose costs do not fit 16 bits, gets a row of 0xFFFF and engine.check()
        raises once.  ValueError for arguments that make no field; nothing is launched then."""
        torch, e = self.torch, self.engine
        if into is not None:
            if not isinstance(into, NavField):
                raise ValueError("nav_field: `into` must be a NavField")
            if into.obstacles == "grid":
                raise ValueError("nav_field: `into` is a grid field: grid_field(into=) rebuilds it")
            if target is not None or margin is not None or reach is not None or (cell, obstacles) != (0.25, "walls"):
                raise ValueError("nav_field: with `into` the field's own target and parameters are used: pass only mask")
            field, params, target = into.field, into.params, into.target
        else:
            flags = self._obstacle_flags("nav_field", obstacles)
            cell, gx, gz = self._grid("nav_field", cell)
            margin = cell / 2 if margin is None else real("nav_field", "margin", margin, lo_open=False)
            if target is None:
                target = int(e.cfg.goal_ent)
                if target < 0:
                    raise ValueError("nav_field: this env has no goal entity: name a target slot or points")
            if torch.is_tensor(target):
                if not self._is_tensor(target, (self.num_envs, 3)):
                    raise ValueError(f"nav_field: point targets are a contiguous float64 tensor [{self.num_envs}, 3] on {e.device}")
                reach = real("nav_field", "reach (point targets need one)", reach)
            elif isinstance(target, (int, np.integer)) and not isinstance(target, bool):
                target = integer("nav_field", "target slot", target, 0, e.cfg.max_ents - 1)
                if reach is not None:
                    raise ValueError("nav_field: a slot target's reach is the env's own near() distance: pass no reach")
            else:
                raise ValueError(f"nav_field: target is None, an entity slot or a float64[N, 3] device tensor, not {type(target).__name__}")
            params = eng.MwNavParams(cell, margin, reach or 0.0, gx, gz, flags, target if isinstance(target, int) else 0)
            # (0xFFFF throughout; filled as int16: the 16-bit unsigned type has few kernels of its own)
            field = torch.full((self.num_envs, gz, gx), -1, dtype=torch.int16, device=e.device).view(torch.uint16)
        mask = self._device_mask(mask, "nav_field")
        out = into if into is not None else NavField(field, params, target, obstacles)
        e.nav_build(params, field, mask, out.points)
        return out

    def _cell_grid(self, where, name, t, gz, gx, optional=True):
        """a grid of bytes of grid_field: None where that may be, or a contiguous uint8 / bool [N, gz, gx] tensor already on the
        device; a bool is viewed as bytes (0 / 1: no conversion kernel)"""
        torch = self.torch
        if t is None and optional:
            return None
        if not any(self._is_tensor(t, (self.num_envs, gz, gx), dt) for dt in (torch.uint8, torch.bool)):
            raise ValueError(f"{where}: {name} is a contiguous uint8 or bool tensor [{self.num_envs}, {gz}, {gx}] on {self.engine.device}")
        return t.view(torch.uint8) if t.dtype == torch.bool else t

    def grid_field(self, blocked, sources=None, target=None, reach=None, extra=None, inflate=None, like=None, cell=0.25, mask=None, into=None):
        """The shortest-path cost to the nearest source over the caller's OWN maps — the planner for a map the agent built from what
        it perceived, where nav_field() reads the simulator's walls —, built on the device by one kernel (mw_nav_build_grid) with no
        host value and no synchronisation: a NavField whose `obstacles` is "grid".  nav_query(), ego_update(source=) and
        seen_map(like=) take it like any other; nav_query's waypoint at cost 0 is the centre of the source cell itself.

        blocked   uint8 or bool [N, gz, gx] device tensor: != 0 a raw obstacle cell (a DepthMap's `obstacle` plane made contiguous, a
                  SeenMap, the caller's own raster)
        sources   the same kind of tensor: != 0 a source cell (a frontier mask: one build gives the way to the nearest frontier)
        target    a float64[N, 3] device tensor of points with `reach` metres around them, as in nav_field(); with `sources` the
                  union of both.  At least one of the two.
        extra     the same kind of tensor as `blocked`: a cost 0 .. 255 added to every path through the cell (sources stay 0)
        inflate   metres: a cell is blocked too when a raw obstacle cell's centre is closer than this to its own.  None:
                  agent_radius + cell / 2, nav_field()'s default clearance.  0: the raw cells only.  At most
                  engine.NAV_MAX_INFLATE cells.  The agent's radius is NOT added: the caller's grid may already hold it.
        like      a NavField, SeenMap, DepthMap, ObjectMap, ScanMap or ScanEvidence whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell` metres
                  per cell as in nav_field().
        mask      uint8[N] or bool[N] device tensor: only those envs' rows are built (the others are not touched)
        into      a grid field to rebuild in place: the grids are passed again, the grid's parameters are the field's own
        The tensors are checked and never converted.  An env whose costs do not fit 16 bits gets a row of 0xFFFF and engine.check()
        raises once.  ValueError for arguments that make no field; nothing is launched then."""
        torch, e = self.torch, self.engine
        if into is not None:
            if not isinstance(into, NavField) or into.obstacles != "grid":
                raise ValueError("grid_field: `into` must be a NavField of grid_field()")
            if target is not None or reach is not None or inflate is not None or like is not None or cell != 0.25:
                raise ValueError("grid_field: with `into` the field's own points and parameters are used: pass only the grids and mask")
            field, params, target = into.field, into.params, into.target
        else:
            g = self._map_grid("grid_field", cell, like, (NavField, SeenMap, DepthMap, ObjectMap, ScanMap, ScanEvidence), "its own")
            cell, gx, gz = g.cell, g.gx, g.gz
            inflate = float(e.cfg.agent_radius) + cell / 2 if inflate is None else real("grid_field", "inflate", inflate, lo_open=False)
            if inflate > eng.NAV_MAX_INFLATE * cell:
                raise ValueError(f"grid_field: inflate {inflate!r} is more than {eng.NAV_MAX_INFLATE} cells of {cell!r}")
            if target is not None:
                if not self._is_tensor(target, (self.num_envs, 3)):
                    raise ValueError(f"grid_field: point targets are a contiguous float64 tensor [{self.num_envs}, 3] on {e.device}")
                reach = real("grid_field", "reach (point targets need one)", reach)
            elif reach is not None:
                raise ValueError("grid_field: reach without point targets")
            params = eng.MwNavParams(cell, inflate, reach or 0.0, gx, gz, eng.NAV_GRID, 0)
        if sources is None and target is None:
            raise ValueError("grid_field: no sources: pass a mask of source cells, point targets, or both")
        blocked = self._cell_grid("grid_field", "blocked", blocked, params.gz, params.gx, optional=False)
        sources = self._cell_grid("grid_field", "sources", sources, params.gz, params.gx)
        extra = self._cell_grid("grid_field", "extra", extra, params.gz, params.gx)
        mask = self._device_mask(mask, "grid_field")
        if into is None:
            # (0xFFFF throughout, as nav_field fills it)
            field = torch.full((self.num_envs, params.gz, params.gx), -1, dtype=torch.int16, device=e.device).view(torch.uint16)
        out = into if into is not None else NavField(field, params, target, "grid")
        e.nav_build_grid(params, field, blocked, sources, target, extra, mask)
        return out

    def nav_query(self, field, pos=None):
        """Where each env's agent — or row i of `pos`, float64[N, 3] on the device — stands in `field` (a NavField), by one small
        kernel (mw_nav_query), no host value: {"cost": int32[N], the cell's cost, -1 where no path leads to the target; "next":
        int32[N], the flat index j * gx + i of the neighbouring cell to go to (-1 without a path); "waypoint": float64[N, 2], that
        cell's centre x, z — the target's own x, z once the cell is a source —; "distance": float32[N], cost * cell / 5 in metres,
        inf where there is no path}.  The distance is the grid's metric — straight and diagonal moves of 5 and 7 — which
        over-estimates the Euclidean geodesic by up to 8 % and is exact along the axes.  A position in a blocked cell (an agent may
        stand closer to a wall than the field's margin) is answered from the best unblocked cell around it.  The tensors are this
        env's own, reused between calls."""
        torch, e = self.torch, self.engine
        if not isinstance(field, NavField):
            raise ValueError("nav_query: `field` must be a NavField (nav_field())")
        if pos is not None and not self._is_tensor(pos, (self.num_envs, 3)):
            raise ValueError(f"nav_query: pos is a contiguous float64 tensor [{self.num_envs}, 3] on {e.device}")
        n = self.num_envs
        b = {name: self._buffer(name, shape, dtype, self._nav_bufs)
             for name, shape, dtype in (("cost", (n,), torch.int32), ("next", (n,), torch.int32), ("waypoint", (n, 2), torch.float64))}
        e.nav_query(field.params, field.field, field.points, pos, b["cost"], b["next"], b["waypoint"])
        dist = torch.where(b["cost"] < 0, float("inf"), b["cost"].to(torch.float32) * (field.cell / 5.0)).to(torch.float32)
        return {"cost": b["cost"], "next": b["next"], "waypoint": b["waypoint"], "distance": dist}

    # ------------------------------------------------------------------ explored-area maps
    def default_fov(self):
        """The horizontal field of view of the default camera in radians: 2 atan(tan(fov_y / 2) * width / height) from the vertical
        field of view the env's parameters default to (cam_fov_y, 60 degrees) and the observation's aspect."""
        cfg = self.engine.cfg
        return 2.0 * math.atan(math.tan(math.radians(float(cfg.cam_fov_y.default)) / 2.0) * float(cfg.obs_width) / float(cfg.obs_height))

    def seen_map(self, cell=0.25, max_range=10.0, fov=None, obstacles="walls", like=None):
        """An empty explored-area map over each env's floor plan: a SeenMap, which seen_update() fills.

        cell       metres per cell; gx, gz follow from the template world's extent exactly as in nav_field()
        like       a NavField (or an ObjectMap) whose grid (cell, gx, gz) the map adopts, so that map and field line up cell for cell; pass
                   no cell then
        max_range  how far the agent sees, in metres
        fov        the horizontal opening angle of sight in radians, 0 < fov <= 2 pi, about the agent's heading; None: default_fov(),
                   the horizontal field of view of the default camera — the vertical field of view the parameters default to and
                   the observation's aspect, so that a cell is seen when the frame could show its floor point.  2 pi: all round.
        obstacles  "walls", or "walls+entities": every listed entity but the carried one blocks the line of sight too, as a disc of
                   full height
        A cell counts as seen once its centre is within max_range and the cone and the straight line from the agent to it meets no
        obstacle (include/mwengine.h, "explored-area maps").  ValueError for arguments that make no map; nothing is launched."""
        torch, e = self.torch, self.engine
        self._obstacle_flags("seen_map", obstacles)
        max_range = real("seen_map", "max_range", max_range)
        cos_half = self._cos_half("seen_map", fov)
        params = self._map_grid("seen_map", cell, like, (NavField, ObjectMap), "the field's own")
        n = self.num_envs
        return SeenMap(torch.zeros((n, params.gz, params.gx), dtype=torch.uint8, device=e.device), torch.zeros(n, dtype=torch.int32, device=e.device),
                       torch.zeros(n, dtype=torch.int32, device=e.device), params, max_range, cos_half, obstacles)

    def seen_update(self, seen, clear=None, mask=None):
        """Marks the cells each env's agent sees from where it stands now in `seen` (a SeenMap), by one kernel (mw_seen_update) with no
        host value and no synchronisation; returns seen.new, int32[N], the cells that became seen in this call, while seen.count
        carries the total.

        clear  uint8[N] or bool[N] device tensor: those envs' rows are zeroed and their counts restarted first.  Behind a step of the
               same-step auto-reset `seen_update(m, clear=terminated | truncated)` starts the map of every new episode with the
               first pose of its world.
        mask   uint8[N] or bool[N] device tensor: only those envs are updated; the rows, counts and `new` of the others are neither
               read nor written, whatever `clear` says.
        An env whose extent the grid does not cover gets its row zeroed and engine.check() raises once.  Tensors are checked, never
        converted: a SeenMap whose tensors were replaced by ones of another shape, dtype or device is refused (EngineError)."""
        if not isinstance(seen, SeenMap):
            raise ValueError("seen_update: `seen` must be a SeenMap (seen_map())")
        clear, mask = self._device_mask(clear, "seen_update", "clear"), self._device_mask(mask, "seen_update")
        self.engine.seen_update(seen.params, seen.max_range, seen.cos_half, self.OBSTACLES[seen.obstacles], seen.seen, seen.count, seen.new, mask, clear)
        return seen.new

    # ------------------------------------------------------------------ grid sight
    def grid_sight(self, opaque, cells=None, dirs=None, weight=None, max_range=3.0, fov=None, like=None, cell=0.25, mask=None, seen=None):
        """What each of V candidate cells per env would see on the caller's OWN map — the gain of a next-best-view planner, where
        seen_update() reads the simulator's walls from the agent's true position —, by one kernel (mw_grid_sight) with no host value and
        no synchronisation: `gain`, int32[N, V], the sum of `weight` over the cells seen from each viewpoint.

        opaque     uint8 or bool [N, gz, gx] device tensor: != 0 a cell that blocks the line of sight (a DepthMap's obstacle plane made
                   contiguous, `field.field == 0xFFFF`, the caller's own raster)
        cells      int32[N, V] device tensor of flat cell indices j * gx + i, 1 <= V <= engine.SIGHT_MAX_VIEWS; a value outside
                   0 .. gx * gz - 1 is no viewpoint: gain 0.  None: V = 1, the agent's own cell and heading
        dirs       float64[N, V] device tensor of headings in radians (as agent_dir), with `cells`; None: every viewpoint looks all round
        weight     the same kind of tensor as `opaque`: what a seen cell is worth, 0 .. 255 (the unknown cells: how much of them each
                   viewpoint would uncover).  None: the count of seen cells
        max_range  how far a viewpoint sees, in metres, centre to centre
        fov        the horizontal opening angle in radians about the heading, 0 < fov <= 2 pi.  None: default_fov() for the agent and
                   with `dirs`; with `cells` and no `dirs` the cone is all round and only None or 2 pi is accepted
        like       a NavField, SeenMap, DepthMap, ObjectMap, ScanMap or ScanEvidence whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell`
                   metres per cell as in nav_field()
        mask       uint8[N] or bool[N] device tensor: only those envs' rows are computed (the others are neither read nor written)
        seen       uint8 or bool [N, gz, gx] device tensor: every cell any viewpoint of the env sees is set to 1; never cleared here
        A cell is seen when its centre is within max_range and the cone of the viewpoint's centre and no opaque cell's closed square
        meets the segment between the two (include/mwengine.h, "grid sight"): a viewpoint sees itself, and an opaque cell's face.
        The tensors are checked and never converted.  ValueError for arguments that make no call; nothing is launched then."""
        torch, e = self.torch, self.engine
        params = self._map_grid("grid_sight", cell, like, (NavField, SeenMap, DepthMap, ObjectMap, ScanMap, ScanEvidence), "its own")
        max_range = real("grid_sight", "max_range", max_range)
        n = self.num_envs
        if cells is None:
            if dirs is not None:
                raise ValueError("grid_sight: dirs without cells: the agent's heading is its own")
            views = 1
            cos_half = self._cos_half("grid_sight", fov)
        else:
            if not self._is_tensor(cells, (n, None), torch.int32) or not 1 <= cells.shape[1] <= eng.SIGHT_MAX_VIEWS:
                raise ValueError(f"grid_sight: cells is a contiguous int32 tensor [{n}, 1 .. {eng.SIGHT_MAX_VIEWS}] on {e.device}")
            views = int(cells.shape[1])
            if dirs is None:
                if fov is not None and fov != 2 * math.pi:
                    raise ValueError("grid_sight: a fov needs headings: pass dirs, or no fov (viewpoints without headings look all round)")
                cos_half = -1.0
            else:
                if not self._is_tensor(dirs, (n, views)):
                    raise ValueError(f"grid_sight: dirs is a contiguous float64 tensor [{n}, {views}] on {e.device}")
                cos_half = self._cos_half("grid_sight", fov)
        opaque = self._cell_grid("grid_sight", "opaque", opaque, params.gz, params.gx, optional=False)
        weight = self._cell_grid("grid_sight", "weight", weight, params.gz, params.gx)
        seen = self._cell_grid("grid_sight", "seen", seen, params.gz, params.gx)
        mask = self._device_mask(mask, "grid_sight")
        gain = torch.zeros((n, views), dtype=torch.int32, device=e.device)
        e.grid_sight(params, max_range, cos_half, views, opaque, gain, weight, cells, dirs, seen, mask)
        return gain

    # ------------------------------------------------------------------ grid regions
    def grid_regions(self, member, connectivity=4, min_cells=1, max_regions=32, like=None, cell=0.25, mask=None, labels=False, sums=True, into=None):
        """The connected regions of a byte mask on the caller's OWN map — a frontier mask's clusters, the cells a field reaches, an
        obstacle plane's specks —, each with its size and one cell of its own to go to, by one kernel (mw_grid_regions) with no host
        value and no synchronisation: a GridRegions.

        member        uint8 or bool [N, gz, gx] device tensor: != 0 a cell of the mask
        connectivity  4: cells that share an edge are joined; 8: cells that share a corner too
        min_cells     regions of fewer cells are not counted and not listed (their cells' label is -1)
        max_regions   K, 1 .. engine.REGION_MAX: the regions listed per env, in the order of their lowest cells; `count` may exceed it
        like          a NavField, SeenMap, DepthMap, ObjectMap, ScanMap or ScanEvidence whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell`
                      metres per cell as in nav_field()
        mask          uint8[N] or bool[N] device tensor: only those envs' rows are computed (the others are neither read nor written)
        labels        with the per-cell `label` plane
        sums          with the per-region `sum` (and `centroid`)
        into          a GridRegions of an earlier call to write into: its grid, connectivity, min_cells, max_regions and optional
                      tensors are used; pass only member and mask
        The representative is the region's cell nearest its centroid, ties to the lowest index (include/mwengine.h, "grid regions").
        The tensors are checked and never converted.  ValueError for arguments that make no call; nothing is launched then."""
        torch, e = self.torch, self.engine
        n = self.num_envs
        if into is not None:
            if not isinstance(into, GridRegions):
                raise ValueError("grid_regions: `into` must be a GridRegions")
            if like is not None or labels is not False or sums is not True or (connectivity, min_cells, max_regions, cell) != (4, 1, 32, 0.25):
                raise ValueError("grid_regions: with `into` the record's own grid and parameters are used: pass only member and mask")
            out, params = into, into.params
        else:
            params = self._map_grid("grid_regions", cell, like, (NavField, SeenMap, DepthMap, ObjectMap, ScanMap, ScanEvidence), "its own")
            if connectivity not in (4, 8) or isinstance(connectivity, bool):
                raise ValueError(f"grid_regions: connectivity {connectivity!r}; have 4 and 8")
            min_cells = integer("grid_regions", "min_cells", min_cells, 1, eng.NAV_MAX_CELLS)
            K = integer("grid_regions", "max_regions", max_regions, 1, eng.REGION_MAX)
            for name, v in (("labels", labels), ("sums", sums)):
                if not isinstance(v, bool):
                    raise ValueError(f"grid_regions: {name} must be True or False, not {v!r}")
        member = self._cell_grid("grid_regions", "member", member, params.gz, params.gx, optional=False)
        mask = self._device_mask(mask, "grid_regions")
        if into is None:
            new = lambda shape, dtype, fill: torch.full(shape, fill, dtype=dtype, device=e.device)
            out = GridRegions(new((n,), torch.int32, 0), new((n, K), torch.int32, 0), new((n, K), torch.int32, -1),
                              new((n, K, 2), torch.int32, 0) if sums else None, new((n, params.gz, params.gx), torch.int16, 0) if labels else None,
                              params, int(connectivity), min_cells)
        e.grid_regions(params, out.connectivity, out.min_cells, out.max_regions, member, out.count, out.size, out.cell, out.sum, out.label, mask)
        return out

    # ------------------------------------------------------------------ grid clearance
    def grid_clearance(self, marked, radii=None, costs=None, limit=None, nearest=False, like=None, cell=0.25, mask=None, into=None):
        """How far every cell of the caller's OWN map is from the nearest marked cell — the exact Euclidean distance transform of an
        obstacle plane, a frontier mask, a seen map —, by one kernel (mw_grid_clearance) with no host value and no synchronisation: a
        GridClearance.

        marked   uint8 or bool [N, gz, gx] device tensor: != 0 a marked cell
        radii    metres, ascending, at most engine.CLEAR_MAX_BANDS, with `costs`, as many integers 0 .. 255: a cell closer than radii[b]
                 to a marked cell's centre, and not closer than radii[b - 1], gets costs[b] in `cost`; 0 from the last radius on.  A
                 radius becomes GridClearance.threshold(radius, cell); a band that holds no distance — its threshold is -1, or not
                 above the one before — is dropped from `bands`.  If that leaves none, `cost` is a plane of zeros the call does not
                 write.
        limit    metres: cells farther than the smallest L cells with L * cell >= limit hold engine.CLEAR_FAR, nearest -1, cost 0, and
                 no scan goes farther: what bounds the work on a nearly empty map.  None: no limit.
        nearest  with the per-cell `nearest` plane
        like     a NavField, SeenMap, DepthMap, ObjectMap, GridRegions, ScanMap or ScanEvidence whose grid (cell, gx, gz) is adopted; pass no cell then.  Else
                 `cell` metres per cell as in nav_field()
        mask     uint8[N] or bool[N] device tensor: only those envs' rows are computed (the others are neither read nor written)
        into     a GridClearance of an earlier call to write into: its grid, bands, limit and optional tensors are used; pass only
                 marked and mask
        The rule in full: include/mwengine.h, "grid clearance".  The tensors are checked and never converted.  ValueError for arguments
        that make no call; nothing is launched then."""
        torch, e = self.torch, self.engine
        where = "grid_clearance"
        if into is not None:
            if not isinstance(into, GridClearance):
                raise ValueError(f"{where}: `into` must be a GridClearance")
            if radii is not None or costs is not None or limit is not None or nearest is not False or like is not None or cell != 0.25:
                raise ValueError(f"{where}: with `into` the record's own grid and parameters are used: pass only marked and mask")
            out, params = into, into.params
        else:
            params = self._map_grid(where, cell, like, (NavField, SeenMap, DepthMap, ObjectMap, GridRegions, ScanMap, ScanEvidence), "its own")
            if not isinstance(nearest, bool):
                raise ValueError(f"{where}: nearest must be True or False, not {nearest!r}")
            if (radii is None) != (costs is None):
                raise ValueError(f"{where}: radii and costs go together")
            bands = []
            if radii is not None:
                if isinstance(radii, (str, bytes)) or isinstance(costs, (str, bytes)) or not all(hasattr(v, "__len__") for v in (radii, costs)):
                    raise ValueError(f"{where}: radii and costs are sequences")
                if len(radii) != len(costs) or not 1 <= len(radii) <= eng.CLEAR_MAX_BANDS:
                    raise ValueError(f"{where}: {len(radii)} radii and {len(costs)} costs: as many of each, 1 .. {eng.CLEAR_MAX_BANDS}")
                radii = [real(where, "a radius", r, lo_open=False) for r in radii]
                if any(b <= a for a, b in zip(radii, radii[1:])):
                    raise ValueError(f"{where}: radii {radii!r} do not ascend")
                for r, c in zip(radii, costs):
                    t, c = GridClearance.threshold(r, params.cell), integer(where, "a cost", c, 0, 255)
                    if t > (bands[-1][0] if bands else -1):         # (else: no distance lies in the band)
                        bands.append((t, c))
            cells = 0
            if limit is not None:
                limit = real(where, "limit", limit)
                cells = int(min(math.ceil(limit / params.cell), 32768.0))       # (from 32768 cells on the call knows no limit: no search)
                while cells < 32768 and cells * params.cell < limit:
                    cells += 1
                while 1 < cells < 32768 and (cells - 1) * params.cell >= limit:
                    cells -= 1
        marked = self._cell_grid(where, "marked", marked, params.gz, params.gx, optional=False)
        mask = self._device_mask(mask, where)
        if into is None:
            new = lambda dtype, fill: torch.full((self.num_envs, params.gz, params.gx), fill, dtype=dtype, device=e.device)
            out = GridClearance(new(torch.int32, eng.CLEAR_NONE), new(torch.int32, -1) if nearest else None, new(torch.uint8, 0) if radii is not None else None,
                                params, tuple(bands), cells)
        e.grid_clearance(params, out.limit, out.bands, marked, out.dist2, out.nearest, out.cost if out.bands else None, mask)
        return out

    # ------------------------------------------------------------------ egocentric map windows
    def ego_window(self, size=33, cell=0.25, anchor="centre", frame="heading", planes=("wall", "entity", "visible"), wall_radius=None,
                   entity_pad=None, max_range=10.0, fov=None, obstacles="walls"):
        """An empty egocentric map window: an EgoWindow, which ego_update() fills.  Nothing is launched.

        size         S: the window is S x S points, 1 .. engine.EGO_MAX_SIZE
        cell         metres between neighbouring points
        anchor       "centre": the agent stands in the window's centre; "bottom": on the middle of its bottom edge, all of it ahead
        frame        "heading": row 0 is the farthest ahead and columns grow to the agent's right; "north": the window keeps the
                     world's axes, rows grow with z and columns with x like every grid here
        planes       which of "wall", "entity", "visible" to compute (kept in that order); () for a window that only samples a source
        wall_radius  a point counts as wall when it is closer than this to a collision segment, or outside the extent; default cell / 2
        entity_pad   added to an entity's radius; default cell / 2
        max_range, fov, obstacles  what "visible" means, exactly as for seen_map()
        ValueError for arguments that make no window."""
        torch, e = self.torch, self.engine
        size, cell, back, frame = self._window_shape("ego_window", size, cell, anchor, frame)
        if isinstance(planes, str) or not isinstance(planes, (tuple, list)) or len(set(planes)) != len(planes) or any(
                not isinstance(p, str) or p not in EgoWindow.PLANES for p in planes):
            raise ValueError(f"ego_window: planes {planes!r}: a sequence of distinct names out of {tuple(EgoWindow.PLANES)}")
        names = tuple(n for n in EgoWindow.PLANES if n in planes)
        if "entity" in names and e.cfg.max_ents > 255:
            raise ValueError(f"ego_window: {e.cfg.max_ents} entity slots do not fit the entity plane's byte")
        wall_radius = cell / 2 if wall_radius is None else real("ego_window", "wall_radius", wall_radius, lo_open=False)
        entity_pad = cell / 2 if entity_pad is None else real("ego_window", "entity_pad", entity_pad, lo_open=False)
        self._obstacle_flags("ego_window", obstacles)
        max_range = real("ego_window", "max_range", max_range)
        cos_half = self._cos_half("ego_window", fov)
        out = torch.zeros((self.num_envs, len(names), size, size), dtype=torch.uint8, device=e.device) if names else None
        return EgoWindow(out, names, size, cell, back, frame, wall_radius, entity_pad, max_range, cos_half, obstacles)

    def ego_update(self, w, source=None, fill=None, mask=None, pos=None):
        """Fills `w` (an EgoWindow) for where each env's agent stands and looks now, by one kernel (mw_ego_map) with no host value and
        no synchronisation; returns w.planes, or (w.planes, sample) with a source.

        source  a SeenMap or a NavField: `sample`, [N, S, S] of the source's dtype (uint8 / uint16), holds the source's cell under
                every point of the window — with the engine's own rounding, so that window and map agree at cell borders.  The
                tensor is this env's own, reused between calls of the same size and dtype.
        fill    what a point outside the source's grid samples; default 0 for a seen map, 0xFFFF (blocked) for a nav field
        mask    uint8[N] or bool[N] device tensor: only those envs' rows are read and written
        pos     float64[N, 3] device tensor: the window's origin instead of the agent's position (y is not read); the heading stays
                the agent's
        Tensors are checked, never converted (EngineError); ValueError for arguments that make no call; nothing is launched then."""
        torch, e = self.torch, self.engine
        if not isinstance(w, EgoWindow):
            raise ValueError("ego_update: `w` must be an EgoWindow (ego_window())")
        src = params = sample = None
        if source is not None:
            if isinstance(source, SeenMap):
                src, limit, default = source.seen, 0xFF, 0
            elif isinstance(source, NavField):
                src, limit, default = source.field, 0xFFFF, eng.NAV_BLOCKED
            else:
                raise ValueError(f"ego_update: source is None, a SeenMap or a NavField, not {type(source).__name__}")
            params = source.params
            fill = default if fill is None else integer("ego_update", "fill", fill, 0, limit)
            if not torch.is_tensor(src):
                raise eng.EngineError(f"ego_update: the source's tensor is {type(src).__name__}")
            sample = self._buffer((w.size, src.dtype), (self.num_envs, w.size, w.size), src.dtype, self._ego_bufs)
        elif fill is not None:
            raise ValueError("ego_update: fill without a source")
        elif not w.names:
            raise ValueError("ego_update: a window without planes needs a source")
        if pos is not None and not self._is_tensor(pos, (self.num_envs, 3)):
            raise ValueError(f"ego_update: pos is a contiguous float64 tensor [{self.num_envs}, 3] on {e.device}")
        mask = self._device_mask(mask, "ego_update")
        flags = self.OBSTACLES[w.obstacles] | (eng.EGO_NORTH if w.frame == "north" else 0)
        e.ego_map(w.size, w.cell, w.back, w.wall_radius, w.entity_pad, w.max_range, w.cos_half, w.bits, flags, w.planes, mask, pos, params, src,
                  fill or 0, sample)
        return w.planes if source is None else (w.planes, sample)

    # ------------------------------------------------------------------ depth projection
    def _depth_sensor(self, where, min_range, max_range, floor_tol, top):
        """(min_range, max_range, floor_tol, top) of a depth window or map, checked"""
        min_range, max_range = real(where, "min_range", min_range), real(where, "max_range", max_range)
        if min_range > max_range:
            raise ValueError(f"{where}: min_range {min_range!r} > max_range {max_range!r}")
        floor_tol = real(where, "floor_tol", floor_tol, lo_open=False)
        top = float(self.engine.cfg.agent_height) if top is None else real(where, "top", top, lo_open=False)
        if top < floor_tol:
            raise ValueError(f"{where}: top {top!r} < floor_tol {floor_tol!r}")
        return min_range, max_range, floor_tol, top

    def _depth_input(self, where, depth):
        """the depth tensor of a projection: the env's own, or the caller's contiguous float32[N, H, W, 1] / [N, H, W] on the device"""
        torch, e = self.torch, self.engine
        if depth is None:
            if self.depth is None:
                raise ValueError(f"{where}: this env draws no depth map: make it with want_depth=True, or pass depth=")
            return self.depth
        n, H, W = self.num_envs, int(e.cfg.obs_height), int(e.cfg.obs_width)
        if not (self._is_tensor(depth, (n, H, W, 1), torch.float32) or self._is_tensor(depth, (n, H, W), torch.float32)):
            raise ValueError(f"{where}: depth is a contiguous float32 tensor [{n}, {H}, {W}, 1] or [{n}, {H}, {W}] on {e.device}")
        return depth

    def _depth_pixel_cap(self, where):
        """a cell's two counts share a 32-bit word in the kernel: frames of more pixels are refused"""
        cfg = self.engine.cfg
        if int(cfg.obs_width) * int(cfg.obs_height) > eng.DEPTH_MAX_PIXELS:
            raise ValueError(f"{where}: frames of {cfg.obs_width} x {cfg.obs_height} pixels > {eng.DEPTH_MAX_PIXELS}")

    def depth_window(self, size=33, cell=0.25, anchor="centre", frame="heading", min_range=0.05, max_range=8.0, floor_tol=0.1, top=None):
        """An empty depth-projected egocentric window: a DepthWindow, which depth_update() fills.  Nothing is launched.

        size, cell, anchor, frame  exactly as for ego_window(): the two windows line up cell for cell
        min_range, max_range       the eye depths in metres whose pixels count.  The depth map steps by z * z * 3.8e-4 metres at depth z
                                   (a 16-bit depth value): 2.4 cm at the default 8 m, a tenth of the default cell; the sky reads 100 and
                                   never counts
        floor_tol                  a point within this of the height of the agent's feet is floor
        top                        a point above floor_tol and up to this height is an obstacle; None: the agent's height — the ceiling
                                   is neither
        ValueError for arguments that make no window."""
        torch, e = self.torch, self.engine
        size, cell, back, frame = self._window_shape("depth_window", size, cell, anchor, frame)
        sensor = self._depth_sensor("depth_window", min_range, max_range, floor_tol, top)
        self._depth_pixel_cap("depth_window")
        out = torch.zeros((self.num_envs, 2, size, size), dtype=torch.uint8, device=e.device)
        return DepthWindow(out, size, cell, back, frame, *sensor)

    def depth_update(self, w, depth=None, mask=None):
        """Fills `w` (a DepthWindow) from a depth map, by one kernel (mw_depth_project) with no host value and no synchronisation;
        returns w.planes.  Every pixel is unprojected with its env's own camera — height, forward displacement, pitch and field of
        view, per env under domain randomisation — at the place inside the pixel where the engine sampled the depth, and with the pose
        the device holds NOW.  That is the pose `self.depth` was drawn for after step(), reset(), a drawn rollout() and the terminal
        step of the next-step mode; it is NOT after a frameless rollout(render=False), whose depth is stale until the next drawn call.

        depth  None: `self.depth` (ValueError without want_depth=True); or a contiguous float32[N, H, W, 1] / [N, H, W] device tensor
        mask   uint8[N] or bool[N] device tensor: only those envs' rows are read and written
        Tensors are checked, never converted (EngineError); ValueError for arguments that make no call; nothing is launched then."""
        if not isinstance(w, DepthWindow):
            raise ValueError("depth_update: `w` must be a DepthWindow (depth_window())")
        depth = self._depth_input("depth_update", depth)
        mask = self._device_mask(mask, "depth_update")
        self.engine.depth_project(depth, w.min_range, w.max_range, w.floor_tol, w.top, mask, size=w.size, cell=w.cell, back=w.back,
                                  flags=eng.EGO_NORTH if w.frame == "north" else 0, planes=w.planes)
        return w.planes

    def depth_map(self, cell=0.25, like=None, min_points=1, min_range=0.05, max_range=8.0, floor_tol=0.1, top=None):
        """An empty depth-built map over each env's floor plan: a DepthMap, which depth_map_update() accumulates.  Nothing is launched.

        cell        metres per cell; gx, gz follow from the template world's extent exactly as in nav_field()
        like        a NavField, SeenMap, ObjectMap, ScanMap or ScanEvidence whose grid (cell, gx, gz) the map adopts, so that they line up cell for cell; pass no
                    cell then
        min_points  how many pixels of ONE depth map must fall into a cell to set it, 1 .. 255
        min_range, max_range, floor_tol, top  as for depth_window()
        At most 16384 cells (the kernel counts in 64 KiB of LDS): ValueError says "use a larger cell" otherwise."""
        torch, e = self.torch, self.engine
        params = self._map_grid("depth_map", cell, like, (NavField, SeenMap, ObjectMap, ScanMap, ScanEvidence), "its own")
        gx, gz = params.gx, params.gz
        if gx * gz > eng.DEPTH_MAX_CELLS:
            raise ValueError(f"depth_map: {gx} x {gz} cells > {eng.DEPTH_MAX_CELLS}: use a larger cell")
        min_points = integer("depth_map", "min_points", min_points, 1, 255)
        sensor = self._depth_sensor("depth_map", min_range, max_range, floor_tol, top)
        self._depth_pixel_cap("depth_map")
        n = self.num_envs
        return DepthMap(torch.zeros((n, 2, gz, gx), dtype=torch.uint8, device=e.device), torch.zeros((n, 2), dtype=torch.int32, device=e.device),
                        torch.zeros((n, 2), dtype=torch.int32, device=e.device), params, min_points, *sensor)

    def depth_map_update(self, m, depth=None, clear=None, mask=None):
        """Accumulates a depth map's points in `m` (a DepthMap), by one kernel (mw_depth_project) with no host value and no
        synchronisation; returns m.new, int32[N, 2], the free and obstacle cells that were set by this call, while m.count carries the
        totals.  The pose is the one the device holds now, as for depth_update() — not the one a frameless rollout left `self.depth` at.

        depth  None: `self.depth`; or a contiguous float32[N, H, W, 1] / [N, H, W] device tensor
        clear  uint8[N] or bool[N] device tensor: those envs' maps are zeroed and their counts restarted first — behind a step of the
               same-step auto-reset, `depth_map_update(m, clear=terminated | truncated)` starts every new episode's map
        mask   uint8[N] or bool[N] device tensor: only those envs are updated; the mask wins over clear
        An env whose extent the grid does not cover gets its map zeroed and engine.check() raises once."""
        if not isinstance(m, DepthMap):
            raise ValueError("depth_map_update: `m` must be a DepthMap (depth_map())")
        depth = self._depth_input("depth_map_update", depth)
        clear, mask = self._device_mask(clear, "depth_map_update", "clear"), self._device_mask(mask, "depth_map_update")
        self.engine.depth_project(depth, m.min_range, m.max_range, m.floor_tol, m.top, mask, params=m.params, min_points=m.min_points, map=m.map,
                                  count=m.count, new=m.new, clear=clear)
        return m.new

    # ------------------------------------------------------------------ scan maps
    def scan_map(self, cell=0.25, like=None, rays=256, fov=2 * math.pi, max_range=10.0, obstacles="walls+entities"):
        """An empty scan-built map over each env's floor plan: a ScanMap, which scan_map_update() accumulates.  Nothing is launched.

        cell       metres per cell; gx, gz follow from the template world's extent exactly as in nav_field()
        like       a NavField, SeenMap, DepthMap, ObjectMap, ScanMap or ScanEvidence whose grid (cell, gx, gz) the map adopts, so that they line up
                   cell for cell; pass no cell then
        rays, fov, obstacles  the lidar() that scan_map_update() casts when it is given no scan
        max_range  metres: a beam is traced up to there, and one that reaches it marks no obstacle"""
        torch, e = self.torch, self.engine
        params = self._map_grid("scan_map", cell, like, (NavField, SeenMap, DepthMap, ObjectMap, ScanMap, ScanEvidence), "its own")
        rays, fov = integer("scan_map", "rays", rays, 1, eng.RAY_MAX), real("scan_map", "fov", fov, hi=2 * math.pi)
        max_range = real("scan_map", "max_range", max_range)
        self._obstacle_flags("scan_map", obstacles)
        n = self.num_envs
        return ScanMap(torch.zeros((n, 2, params.gz, params.gx), dtype=torch.uint8, device=e.device), torch.zeros((n, 2), dtype=torch.int32, device=e.device),
                       torch.zeros((n, 2), dtype=torch.int32, device=e.device), params, rays, fov, max_range, obstacles)

    def scan_map_update(self, m, scan=None, origin=None, clear=None, mask=None):
        """Traces a range scan's beams into `m` (a ScanMap), by one kernel (mw_scan_project) with no host value and no synchronisation:
        the cells a beam passes through become free, the cell a beam shorter than m.max_range ends in becomes an obstacle (and is not
        free in this call); returns m.new, int32[N, 2], the free and obstacle cells that were set by this call, while m.count carries
        the totals.  It needs no frame: behind rollout(render=False) the map is as current as the pose.

        scan    None: `self.lidar(m.rays, m.fov, m.max_range, obstacles=m.obstacles)`, cast now; or a raycast() / lidar() result, or any
                dict with contiguous float64 "t" [N, R] and "dir" [N, R, 2] (dx, dz, any length) on the device — the caller's own
                beams: with noise, with dropped ones (a NaN or a negative t), R up to engine.RAY_MAX.  Checked, never converted
        origin  float64[N, 3] device tensor (y is not read), the beams' origin per env — a pose estimate; None: the agents' positions
                the device holds now
        clear   uint8[N] or bool[N] device tensor: those envs' maps are zeroed and their counts restarted first
        mask    uint8[N] or bool[N] device tensor: only those envs are updated; the mask wins over clear
        The rule in full: include/mwengine.h, "scan maps".  An env whose extent the grid does not cover gets its map zeroed and
        engine.check() raises once.  ValueError for arguments that make no call; nothing is launched then."""
        if not isinstance(m, ScanMap):
            raise ValueError("scan_map_update: `m` must be a ScanMap (scan_map())")
        scan, clear, mask = self._scan_update_args("scan_map_update", m, scan, origin, clear, mask)
        self.engine.scan_project(m.params, m.max_range, scan["t"], scan["dir"], m.map, m.count, m.new, origin, mask, clear)
        return m.new

    def _scan_update_args(self, where, m, scan, origin, clear, mask):
        """(scan, clear, mask) of scan_map_update() and scan_evidence_update(), checked and never converted; a None scan is `m`'s own
        lidar(), cast once everything else is known to be right"""
        e, n = self.engine, self.num_envs
        if scan is not None:
            if not isinstance(scan, dict) or "t" not in scan or "dir" not in scan:
                raise ValueError(f'{where}: `scan` is a dict with "t" and "dir" (a lidar() result, or raycast()\'s with the directions beside it)')
            if not self._is_tensor(scan["t"], (n, None)) or not 1 <= scan["t"].shape[1] <= eng.RAY_MAX:
                raise ValueError(f'{where}: scan["t"] is a contiguous float64 tensor [{n}, R] on {e.device}, R in 1 .. {eng.RAY_MAX}')
            if not self._is_tensor(scan["dir"], (n, int(scan["t"].shape[1]), 2)):
                raise ValueError(f'{where}: scan["dir"] is a contiguous float64 tensor [{n}, {int(scan["t"].shape[1])}, 2] on {e.device}')
        if origin is not None and not self._is_tensor(origin, (n, 3)):
            raise ValueError(f"{where}: origin is a contiguous float64 tensor [{n}, 3] on {e.device}")
        clear, mask = self._device_mask(clear, where, "clear"), self._device_mask(mask, where)
        if scan is None:
            scan = self.lidar(m.rays, m.fov, m.max_range, obstacles=m.obstacles)
        return scan, clear, mask

    # ------------------------------------------------------------------ scan evidence
    def scan_evidence(self, cell=0.25, like=None, rays=256, fov=2 * math.pi, max_range=10.0, obstacles="walls+entities", hit=3, miss=1, cap=1, lo=-20, hi=20,
                      free_at=-1, occ_at=1):
        """An empty evidence map over each env's floor plan: a ScanEvidence, which scan_evidence_update() accumulates.  Nothing is launched.

        cell, like, rays, fov, max_range, obstacles  as for scan_map(); `like` may also be a ScanEvidence
        hit, miss  0 .. 127: what a cell gains per beam that ends in it, loses per beam that passes through it
        cap        1 .. engine.RAY_MAX: the beams of one scan that count per cell — 1: a scan votes once per cell
        lo, hi     -127 .. -1 and 1 .. 127: the clamp; with the defaults seven clean misses retract a cell twenty hits built
        free_at, occ_at  lo .. -1 and 1 .. hi: a cell is free at or below the first, an obstacle at or above the second"""
        torch, e, where = self.torch, self.engine, "scan_evidence"
        params = self._map_grid(where, cell, like, (NavField, SeenMap, DepthMap, ObjectMap, ScanMap, ScanEvidence), "its own")
        rays, fov = integer(where, "rays", rays, 1, eng.RAY_MAX), real(where, "fov", fov, hi=2 * math.pi)
        max_range = real(where, "max_range", max_range)
        self._obstacle_flags(where, obstacles)
        hit, miss, cap = integer(where, "hit", hit, 0, 127), integer(where, "miss", miss, 0, 127), integer(where, "cap", cap, 1, eng.RAY_MAX)
        lo, hi = integer(where, "lo", lo, -127, -1), integer(where, "hi", hi, 1, 127)
        free_at, occ_at = integer(where, "free_at", free_at, lo, -1), integer(where, "occ_at", occ_at, 1, hi)
        n, zeros = self.num_envs, lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=e.device)      # noqa: E731
        return ScanEvidence(zeros((n, params.gz, params.gx), torch.int8), zeros((n, 2, params.gz, params.gx), torch.uint8), zeros((n, params.gz, params.gx), torch.uint8),
                            zeros((n, 2), torch.int32), zeros((n, 2), torch.int32), params, rays, fov, max_range, obstacles, (hit, miss, cap, lo, hi, free_at, occ_at))

    def scan_evidence_update(self, m, scan=None, origin=None, clear=None, mask=None):
        """Counts a range scan's beams into `m` (a ScanEvidence), by one kernel (mw_scan_evidence) with no host value and no
        synchronisation: a cell where beams shorter than m.max_range end gains m.hit per beam, any other cell loses m.miss per beam
        that passes through it, either for at most m.cap beams, and m.ev is clamped to m.lo .. m.hi; m.map, m.score and m.count are
        rewritten from it.  Returns m.changed, int32[N, 2]: the cells that joined or left the free and the obstacle plane.  Unlike a
        ScanMap, a later scan takes back what an earlier one got wrong.

        scan, origin, clear, mask  as for scan_map_update(): the same checks; under `clear` the evidence restarts from 0
        The rule in full: include/mwengine.h, "scan evidence".  An env whose extent the grid does not cover gets its planes zeroed and
        engine.check() raises once.  ValueError for arguments that make no call; nothing is launched then."""
        if not isinstance(m, ScanEvidence):
            raise ValueError("scan_evidence_update: `m` must be a ScanEvidence (scan_evidence())")
        scan, clear, mask = self._scan_update_args("scan_evidence_update", m, scan, origin, clear, mask)
        self.engine.scan_evidence(m.params, m.max_range, m.rule, scan["t"], scan["dir"], m.ev, m.count, m.map, m.score, m.changed, origin, mask, clear)
        return m.changed

    # ------------------------------------------------------------------ scan matching
    def scan_match(self, score, scan, origin=None, window=8, turn=0.0, turns=1, max_range=10.0, like=None, cell=0.25, mask=None, volume=False, into=None):
        """Aligns a range scan to the caller's OWN map — Olson's brute-force correlative scan matcher, what corrects the pose estimate
        that scan_map_update(origin=) takes —, by one kernel (mw_scan_match) with no host value and no synchronisation: a ScanMatch.
        Every candidate (rotation, a, b) is scored by the sum of `score`'s bytes under the end cells of the scan's beams, turned by the
        rotation about `origin` and shifted by (a, b) whole cells; the highest score wins, ties go to the smallest shift, then turn.

        score      uint8[N, gz, gx] contiguous device tensor, the likelihood plane: an obstacle plane made contiguous (bytes 0 / 1), or
                   better a banded field around it, grid_clearance(m.obstacle != 0, radii, costs).cost.  Checked, never converted
        scan       a raycast() / lidar() result, or any dict with contiguous float64 "t" [N, R] and "dir" [N, R, 2] on the device, as
                   for scan_map_update(); only beams with 0 <= t < max_range count
        origin     float64[N, 3] device tensor (y is not read): the pose estimate's position; None: the agents' positions
        window     W, 0 .. engine.MATCH_MAX_WINDOW: shifts of -W .. W cells either way
        turn, turns  the rotations: `turns` of them, an odd number up to engine.MATCH_MAX_ROT, evenly over -turn .. +turn radians
                   about the scan as given (cos and sin are taken on the host); turns = 1: no rotation, and turn must be 0
        max_range  metres: a beam that reached it has no end point
        like       a map or field whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell` metres per cell as in nav_field()
        mask       uint8[N] or bool[N] device tensor: only those envs' rows are computed (the others are neither read nor written)
        volume     with the score of every candidate, int32[N, turns, 2 W + 1, 2 W + 1]
        into       a ScanMatch of an earlier call to write into: its grid, window, rotations, max_range and volume are used; pass only
                   score, scan, origin and mask
        The rule in full: include/mwengine.h, "scan matching".  An env whose extent the grid does not cover gets zeros and
        engine.check() raises once.  ValueError for arguments that make no call; nothing is launched then."""
        out, origin, mask = self._scan_align("scan_match", eng.MATCH_MAX_WINDOW, (8, False), "volume", score, scan, origin, window, turn, turns, max_range, like, cell,
                                             mask, volume, into)
        self.engine.scan_match(out.params, out.max_range, out.pairs, out.window, score, scan["t"], scan["dir"], out.best, out.score, out.volume, origin, mask)
        return out

    def _scan_align(self, where, max_window, defaults, extra_name, score, scan, origin, window, turn, turns, max_range, like, cell, mask, extra, into):
        """scan_match's and scan_search's argument rules, which differ in the window's limit and in the one extra tensor (`extra`, a
        bool: the volume, the stats): (the ScanMatch to fill — `into`, or a new one, with the extra tensor where asked —, origin, mask)"""
        torch, e, n = self.torch, self.engine, self.num_envs
        searched = extra_name == "stats"
        if into is not None:
            if not isinstance(into, ScanMatch):
                raise ValueError(f"{where}: `into` must be a ScanMatch")
            if hasattr(into, "stats") != searched:
                raise ValueError(f"{where}: `into` must be a ScanMatch of {where}, not of " + ("scan_match" if searched else "scan_search"))
            if (window, turn, turns, max_range, like, cell, extra) != (defaults[0], 0.0, 1, 10.0, None, 0.25, defaults[1]):
                raise ValueError(f"{where}: with `into` the record's own grid and parameters are used: pass only score, scan, origin and mask")
            out = into
        else:
            params = self._map_grid(where, cell, like, (NavField, SeenMap, DepthMap, ObjectMap, GridRegions, GridClearance, ScanMap, ScanEvidence), "its own")
            window = integer(where, "window", window, 0, max_window)
            turns = integer(where, "turns", turns, 1, eng.MATCH_MAX_ROT)
            turn = real(where, "turn", turn, hi=math.pi, lo_open=False)
            if turns % 2 == 0 or (turns == 1) != (turn == 0.0):
                raise ValueError(f"{where}: turns {turns} and turn {turn!r}: an odd count, and 1 exactly with turn = 0")
            max_range = real(where, "max_range", max_range)
            if not isinstance(extra, bool):
                raise ValueError(f"{where}: {extra_name} must be True or False, not {extra!r}")
            d = turn / (turns // 2) if turns > 1 else 0.0
            angles = [0.0] + [sign * k * d for k in range(1, turns // 2 + 1) for sign in (1.0, -1.0)]
            rot = [(math.cos(a), math.sin(a)) for a in angles]
        gz, gx = (out.gz, out.gx) if into is not None else (params.gz, params.gx)
        if not self._is_tensor(score, (n, gz, gx), torch.uint8):
            raise ValueError(f"{where}: score is a contiguous uint8 tensor [{n}, {gz}, {gx}] on {e.device}")
        if not isinstance(scan, dict) or "t" not in scan or "dir" not in scan:
            raise ValueError(f'{where}: `scan` is a dict with "t" and "dir" (a lidar() result, or raycast()\'s with the directions beside it)')
        if not self._is_tensor(scan["t"], (n, None)) or not 1 <= scan["t"].shape[1] <= eng.RAY_MAX:
            raise ValueError(f'{where}: scan["t"] is a contiguous float64 tensor [{n}, R] on {e.device}, R in 1 .. {eng.RAY_MAX}')
        if not self._is_tensor(scan["dir"], (n, int(scan["t"].shape[1]), 2)):
            raise ValueError(f'{where}: scan["dir"] is a contiguous float64 tensor [{n}, {int(scan["t"].shape[1])}, 2] on {e.device}')
        if origin is not None and not self._is_tensor(origin, (n, 3)):
            raise ValueError(f"{where}: origin is a contiguous float64 tensor [{n}, 3] on {e.device}")
        mask = self._device_mask(mask, where)
        if into is None:
            side = 2 * window + 1
            out = ScanMatch(torch.zeros((n, 3), dtype=torch.int32, device=e.device), torch.zeros(n, dtype=torch.int32, device=e.device),
                            torch.zeros((n, turns, side, side), dtype=torch.int32, device=e.device) if extra and not searched else None,
                            torch.tensor(angles, dtype=torch.float64, device=e.device), torch.tensor(rot, dtype=torch.float64, device=e.device), rot, window, params, max_range)
            if searched:
                out.stats = torch.zeros((n, 2), dtype=torch.int32, device=e.device) if extra else None
        return out, origin, mask

    # ------------------------------------------------------------------ scan search
    def scan_search(self, score, scan, origin=None, window=64, turn=0.0, turns=1, max_range=10.0, like=None, cell=0.25, mask=None, stats=False, into=None):
        """scan_match() over a wide window — closing a loop after drift, finding an agent again after a teleport or a lost track, matching
        over the whole turn — by one kernel (mw_scan_search) with no host value and no synchronisation: a ScanMatch with `best` and
        `score` exactly as scan_match() would give them for the same arguments, and `volume` None, so offset() and apply() work as they
        are.  Instead of scoring every candidate, the kernel bounds blocks of 8 x 8 translations from above and scores only the blocks
        that can still win (Olson's multi-resolution search, Cartographer's branch and bound); a skipped block provably holds no winner.

        score, scan, origin, turn, turns, max_range, like, cell, mask    as for scan_match()
        window     W, 0 .. engine.SEARCH_MAX_WINDOW: shifts of -W .. W cells either way
        stats      with `stats`, int32[N, 2], an attribute of the result: the blocks the kernel scored — this number depends on its
                   schedule, nothing else does — and the blocks in all, turns * ceil((2 W + 1) / 8)^2
        into       a ScanMatch of an earlier scan_search() to write into; pass only score, scan, origin and mask
        On a constant plane every candidate ties and nothing is skipped: the cost is scan_match()'s and the bounds on top.  More than
        engine.MATCH_MAX_ROT rotations: chain calls and compare the scores.  The rule: include/mwengine.h, "scan search"."""
        out, origin, mask = self._scan_align("scan_search", eng.SEARCH_MAX_WINDOW, (64, False), "stats", score, scan, origin, window, turn, turns, max_range, like, cell,
                                             mask, stats, into)
        self.engine.scan_search(out.params, out.max_range, out.pairs, out.window, score, scan["t"], scan["dir"], out.best, out.score, out.stats, origin, mask)
        return out

    # ------------------------------------------------------------------ scan weighing and resampling
    def scan_weigh(self, score, scan, poses, max_range=10.0, like=None, cell=0.25, mask=None, into=None):
        """Scores a range scan on the caller's OWN map from P free poses per env — the likelihood-field measurement update of Monte Carlo
        localisation —, by one kernel (mw_scan_weigh) with no host value and no synchronisation: a ScanWeights.  A particle's score is
        the sum of `score`'s bytes under the end cells of the scan's beams, turned by the particle's angle about its position.

        score      uint8[N, gz, gx] contiguous device tensor, the likelihood plane, as for scan_match().  Checked, never converted
        scan       a raycast() / lidar() result, or any dict with contiguous float64 "t" [N, R] and "dir" [N, R, 2] on the device; only
                   beams with 0 <= t < max_range count
        poses      float64[N, P, 3] device tensor of (x, z, turn), P in 1 .. engine.WEIGH_MAX_PARTICLES; turn in radians in the sense of
                   scan_match()'s rotations (torch takes cos and sin on the device); a NaN pose scores 0.  [N, P, 4] is taken too: the
                   fourth column is the caller's own and is not read, so that resample() moves the same rows
        max_range  metres: a beam that reached it has no end point
        like       a map or field whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell` metres per cell as in nav_field()
        mask       uint8[N] or bool[N] device tensor: only those envs' rows are computed (the others are neither read nor written)
        into       a ScanWeights of an earlier call with as many particles to write into: its grid and max_range are used
        The rule in full: include/mwengine.h, "scan weighing and resampling".  An env whose extent the grid does not cover gets zeros
        and engine.check() raises once.  ValueError for arguments that make no call; nothing is launched then."""
        torch, e, n, where = self.torch, self.engine, self.num_envs, "scan_weigh"
        if into is not None:
            if not isinstance(into, ScanWeights):
                raise ValueError(f"{where}: `into` must be a ScanWeights")
            if (max_range, like, cell) != (10.0, None, 0.25):
                raise ValueError(f"{where}: with `into` the record's own grid and max_range are used: pass only score, scan, poses and mask")
            params, max_range = into.params, into.max_range
        else:
            params = self._map_grid(where, cell, like, (NavField, SeenMap, DepthMap, ObjectMap, GridRegions, GridClearance, ScanMap, ScanEvidence, ScanMatch, ScanWeights), "its own")
            max_range = real(where, "max_range", max_range)
        if not self._is_tensor(score, (n, params.gz, params.gx), torch.uint8):
            raise ValueError(f"{where}: score is a contiguous uint8 tensor [{n}, {params.gz}, {params.gx}] on {e.device}")
        if not isinstance(scan, dict) or "t" not in scan or "dir" not in scan:
            raise ValueError(f'{where}: `scan` is a dict with "t" and "dir" (a lidar() result, or raycast()\'s with the directions beside it)')
        if not self._is_tensor(scan["t"], (n, None)) or not 1 <= scan["t"].shape[1] <= eng.RAY_MAX:
            raise ValueError(f'{where}: scan["t"] is a contiguous float64 tensor [{n}, R] on {e.device}, R in 1 .. {eng.RAY_MAX}')
        if not self._is_tensor(scan["dir"], (n, int(scan["t"].shape[1]), 2)):
            raise ValueError(f'{where}: scan["dir"] is a contiguous float64 tensor [{n}, {int(scan["t"].shape[1])}, 2] on {e.device}')
        if not (self._is_tensor(poses, (n, None, 3)) or self._is_tensor(poses, (n, None, 4))) or not 1 <= poses.shape[1] <= eng.WEIGH_MAX_PARTICLES:
            raise ValueError(f"{where}: poses is a contiguous float64 tensor [{n}, P, 3] (or 4) on {e.device}, P in 1 .. {eng.WEIGH_MAX_PARTICLES}")
        particles = int(poses.shape[1])
        if into is not None and into.pose.shape[1] != particles:
            raise ValueError(f"{where}: `into` holds {int(into.pose.shape[1])} particles per env, poses {particles}")
        mask = self._device_mask(mask, where)
        if into is None:
            zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=e.device)      # noqa: E731
            into = ScanWeights(zeros(n, particles), zeros(n, particles), zeros(n, 2), torch.empty((n, particles, 4), dtype=torch.float64, device=e.device),
                               params, max_range)
        into.pose[..., :2] = poses[..., :2]
        torch.cos(poses[..., 2], out=into.pose[..., 2])
        torch.sin(poses[..., 2], out=into.pose[..., 3])
        e.scan_weigh(into.params, into.max_range, score, scan["t"], scan["dir"], into.pose, into.score, into.inside, into.best, mask)
        return into

    def resample(self, weights, offset=None, poses=None, mask=None, into=None):
        """Draws the next generation of particles from their weights — systematic (low-variance) resampling in integers —, by one kernel
        (mw_resample) with no host value and no synchronisation: {"ancestor": int32[N, P], the particle each new one descends from,
        non-decreasing; "pose": the ancestors' rows of `poses`, or None}.  Particle p is drawn floor or ceil of P w_p / sum(w) times; a
        row of zero weights keeps every particle.

        weights    int64[N, P] or int32[N, P] contiguous device tensor, P in 1 .. engine.WEIGH_MAX_PARTICLES, of integers in 0 .. 2^32 - 1:
                   the dtype and shape are checked, the values are brought into that range on the device (no value is read on the
                   host) and converted to the kernel's unsigned words once
        offset     int64[N] device tensor, read as unsigned: where in the first stratum the comb starts (taken modulo the sum); None:
                   drawn with torch's generator on the device
        poses      float64[N, P, 4] contiguous device tensor: the rows to move, four doubles each as they are — scan_weigh()'s `poses` in
                   its four-column form (x, z, turn and a column of the caller's own), or a ScanWeights.pose
        mask       uint8[N] or bool[N] device tensor: only those envs' rows are computed (the others are neither read nor written)
        into       the dict of an earlier call of the same shapes to write into
        The rule in full: include/mwengine.h, "scan weighing and resampling".  ValueError for arguments that make no call."""
        torch, e, n, where = self.torch, self.engine, self.num_envs, "resample"
        if not (self._is_tensor(weights, (n, None), torch.int64) or self._is_tensor(weights, (n, None), torch.int32)) or not 1 <= weights.shape[1] <= eng.WEIGH_MAX_PARTICLES:
            raise ValueError(f"{where}: weights is a contiguous int64 or int32 tensor [{n}, P] on {e.device}, P in 1 .. {eng.WEIGH_MAX_PARTICLES}")
        particles = int(weights.shape[1])
        if offset is not None and not self._is_tensor(offset, (n,), torch.int64):
            raise ValueError(f"{where}: offset is a contiguous int64 tensor [{n}] on {e.device}")
        if poses is not None and not self._is_tensor(poses, (n, particles, 4)):
            raise ValueError(f"{where}: poses is a contiguous float64 tensor [{n}, {particles}, 4] on {e.device}")
        mask = self._device_mask(mask, where)
        if into is not None:
            if (not isinstance(into, dict) or not self._is_tensor(into.get("ancestor"), (n, particles), torch.int32)
                    or (into.get("pose") is None) != (poses is None) or (poses is not None and not self._is_tensor(into["pose"], (n, particles, 4)))):
                raise ValueError(f"{where}: `into` is the result of an earlier call with weights and poses of these shapes")
            if poses is not None and into["pose"].data_ptr() == poses.data_ptr():
                raise ValueError(f"{where}: `into` holds `poses` itself: the rows move between two buffers")
        else:
            into = {"ancestor": torch.zeros((n, particles), dtype=torch.int32, device=e.device), "pose": None if poses is None else torch.zeros_like(poses)}
        if weights.dtype == torch.int64:        # (the low words of the clamped values: the unsigned 32 bits the kernel reads)
            words = weights.clamp(0, 2 ** 32 - 1).view(torch.int32)[:, 0::2].contiguous()
        else:
            words = weights.clamp(min=0)
        if offset is None:
            offset = torch.randint(0, 2 ** 63 - 1, (n,), dtype=torch.int64, device=e.device)
        e.resample(words, offset, into["ancestor"], poses, into["pose"], mask)
        return into

    # ------------------------------------------------------------------ label frames
    MESHES = {"exact": eng.LABEL_MESH_EXACT, "bounds": eng.LABEL_MESH_BOUNDS}

    def label_frame(self, meshes="exact", code=True, depth=False, stats=False, near=0.04, far=100.0):
        """An empty label frame: a LabelFrame, which label_update() fills.  Nothing is launched.

        meshes     "exact": a mesh object (ball, key, ...) is labelled where its own triangles show; "bounds": where its bounding cylinder
                   does — cheaper, and a little wider than the object
        code       with the per-pixel codes (and `slot`); False: the class plane alone
        depth      with the per-pixel eye depth
        stats      with the per-slot pixel counts and boxes (detection targets)
        near, far  the eye depths a hit may have; the defaults are the frame's own planes
        ValueError for arguments that make no frame."""
        torch, e = self.torch, self.engine
        if not isinstance(meshes, str) or meshes not in self.MESHES:
            raise ValueError(f"label_frame: meshes {meshes!r}; have {sorted(self.MESHES)}")
        for name, v in (("code", code), ("depth", depth), ("stats", stats)):
            if not isinstance(v, bool):
                raise ValueError(f"label_frame: {name} must be True or False, not {v!r}")
        near, far = real("label_frame", "near", near, lo_open=False), real("label_frame", "far", far)
        if near >= far:
            raise ValueError(f"label_frame: near {near!r} >= far {far!r}")
        n, H, W, E = self.num_envs, int(e.cfg.obs_height), int(e.cfg.obs_width), int(e.E)
        new = lambda shape, dtype, fill: torch.full(shape, fill, dtype=dtype, device=e.device)
        box = None
        if stats:
            box = torch.tensor([W, H, -1, -1], dtype=torch.int32, device=e.device).repeat(n, E, 1)
        return LabelFrame(new((n, H, W), torch.uint8, 0), new((n, H, W), torch.int32, -1) if code else None,
                          new((n, H, W), torch.float32, far) if depth else None, new((n, E), torch.int32, 0) if stats else None, box, meshes, near, far)

    def label_update(self, f, mask=None):
        """Fills `f` (a LabelFrame) with what every pixel of the current observation shows, by one kernel (mw_label_frame) with no host
        value and no synchronisation; returns f.cls.  The label of a pixel is the first thing the ray through the pixel's depth sample
        meets — a static polygon as drawn, a Box, a mesh object —, cast in float64 with each env's own camera and the pose the device
        holds NOW (the one `vec.obs` was drawn for after step(), reset() and a drawn rollout()).  The carried object is drawn, so it is
        labelled.  Nothing of the engine changes.

        mask   uint8[N] or bool[N] device tensor: only those envs' rows are read and written
        Tensors are checked, never converted (EngineError); ValueError for arguments that make no call; nothing is launched then."""
        if not isinstance(f, LabelFrame):
            raise ValueError("label_update: `f` must be a LabelFrame (label_frame())")
        mask = self._device_mask(mask, "label_update")
        params = eng.MwLabelParams(f.near, f.far, self.MESHES[f.meshes], 0)
        self.engine.label_frame(params, f.cls, f.code, f.depth, f.ent_pixels, f.ent_box, mask)
        return f.cls

    # ------------------------------------------------------------------ object maps
    def _label_input(self, where, labels, depth):
        """(code, base, depth) of an object projection: a LabelFrame with `code` — ids are its entity slots, and its own depth serves where
        it has one — or the caller's contiguous int32[N, H, W] category image on the device — ids are its values"""
        torch, e = self.torch, self.engine
        n, H, W = self.num_envs, int(e.cfg.obs_height), int(e.cfg.obs_width)
        if isinstance(labels, LabelFrame):
            if labels.code is None:
                raise ValueError(f"{where}: the label frame has no `code`: make it with label_frame(code=True)")
            code, base = labels.code, eng.RAY_ENT
            if depth is None and labels.depth is not None:
                depth = labels.depth
        elif torch.is_tensor(labels):
            code, base = labels, 0
        else:
            raise ValueError(f"{where}: labels is a LabelFrame or an int32 tensor [{n}, {H}, {W}] on {e.device}, not {type(labels).__name__}")
        if not self._is_tensor(code, (n, H, W), torch.int32):
            raise ValueError(f"{where}: the labels are a contiguous int32 tensor [{n}, {H}, {W}] on {e.device}")
        return code, base, self._depth_input(where, depth)

    def object_window(self, size=33, cell=0.25, anchor="centre", frame="heading", min_range=0.05, max_range=8.0, floor_tol=0.1, top=None):
        """An empty sensed object window: an ObjectWindow, which object_update() fills.  Nothing is launched.  Every argument is
        depth_window()'s: the two windows, and an ego_window()'s entity plane, line up cell for cell.
        ValueError for arguments that make no window."""
        torch, e = self.torch, self.engine
        size, cell, back, frame = self._window_shape("object_window", size, cell, anchor, frame)
        sensor = self._depth_sensor("object_window", min_range, max_range, floor_tol, top)
        self._depth_pixel_cap("object_window")
        return ObjectWindow(torch.zeros((self.num_envs, size, size), dtype=torch.uint8, device=e.device), size, cell, back, frame, *sensor)

    def object_update(self, w, labels, depth=None, mask=None):
        """Fills `w` (an ObjectWindow) from a label image and a depth map, by one kernel (mw_label_project) with no host value and no
        synchronisation; returns w.plane.  Every pixel that depth_update() would count — unprojected with its env's own camera and the pose
        the device holds NOW — writes its id into the cell it falls in; the lowest id wins a shared cell.

        labels  a LabelFrame with `code` (label_update() filled it): ids are entity slots, 0 .. 254; or a contiguous int32[N, H, W] device
                tensor, the caller's own category image (a segmenter's arg-max): ids are its values 0 .. 254, anything else is no object
        depth   None: the label frame's own `depth` where it has one, else `self.depth`; or a contiguous float32[N, H, W, 1] / [N, H, W]
                device tensor
        mask    uint8[N] or bool[N] device tensor: only those envs' rows are read and written
        Tensors are checked, never converted (EngineError); ValueError for arguments that make no call; nothing is launched then."""
        if not isinstance(w, ObjectWindow):
            raise ValueError("object_update: `w` must be an ObjectWindow (object_window())")
        code, base, depth = self._label_input("object_update", labels, depth)
        mask = self._device_mask(mask, "object_update")
        self.engine.label_project(depth, code, base, w.min_range, w.max_range, w.floor_tol, w.top, mask, size=w.size, cell=w.cell, back=w.back,
                                  flags=eng.EGO_NORTH if w.frame == "north" else 0, plane=w.plane)
        return w.plane

    def object_map(self, cell=0.25, like=None, ids=None, min_range=0.05, max_range=8.0, floor_tol=0.1, top=None):
        """An empty sensed object map over each env's floor plan: an ObjectMap, which object_map_update() keeps.  Nothing is launched.

        cell   metres per cell; gx, gz follow from the template world's extent exactly as in nav_field()
        like   a NavField, SeenMap, DepthMap, ObjectMap, ScanMap or ScanEvidence whose grid (cell, gx, gz) the map adopts, so that they line up cell for cell; pass
               no cell then
        ids    K, 0 .. 255: `cells` and `pos` have a row for each id below it (an id from K on is mapped, not counted); None: the env's
               entity slots, at most 255.  0: the map alone
        min_range, max_range, floor_tol, top  as for depth_window()
        At most 16384 cells (the kernel keeps a key per cell in LDS): ValueError says "use a larger cell" otherwise."""
        torch, e = self.torch, self.engine
        params = self._map_grid("object_map", cell, like, (NavField, SeenMap, DepthMap, ObjectMap, ScanMap, ScanEvidence), "its own")
        gx, gz = params.gx, params.gz
        if gx * gz > eng.LABELMAP_MAX_CELLS:
            raise ValueError(f"object_map: {gx} x {gz} cells > {eng.LABELMAP_MAX_CELLS}: use a larger cell")
        ids = min(int(e.cfg.max_ents), eng.LABELMAP_MAX_IDS) if ids is None else integer("object_map", "ids", ids, 0, eng.LABELMAP_MAX_IDS)
        sensor = self._depth_sensor("object_map", min_range, max_range, floor_tol, top)
        self._depth_pixel_cap("object_map")
        n = self.num_envs
        return ObjectMap(torch.zeros((n, gz, gx), dtype=torch.uint8, device=e.device), torch.zeros((n, ids), dtype=torch.int32, device=e.device),
                         torch.full((n, ids, 3), float("nan"), dtype=torch.float64, device=e.device), params, ids, *sensor)

    def object_map_update(self, m, labels, depth=None, clear=None, mask=None):
        """Writes what a label image and a depth map show into `m` (an ObjectMap), by one kernel (mw_label_project) with no host value and
        no synchronisation; returns m.cells, int32[N, ids], while m.pos carries each id's centroid.  The last observation wins: a cell
        this frame saw gets the lowest id of its pixels or 0, every other cell keeps its byte.  The pose is the one the device holds
        now, as for depth_map_update().

        labels, depth  as for object_update()
        clear  uint8[N] or bool[N] device tensor: those envs' maps are rewritten whole — behind a step of the same-step auto-reset,
               `object_map_update(m, labels, clear=terminated | truncated)` starts every new episode's map
        mask   uint8[N] or bool[N] device tensor: only those envs are updated; the mask wins over clear
        An env whose extent the grid does not cover gets its map zeroed, its cells 0 and its positions NaN, and engine.check() raises once."""
        if not isinstance(m, ObjectMap):
            raise ValueError("object_map_update: `m` must be an ObjectMap (object_map())")
        code, base, depth = self._label_input("object_map_update", labels, depth)
        clear, mask = self._device_mask(clear, "object_map_update", "clear"), self._device_mask(mask, "object_map_update")
        ids = int(m.ids)
        self.engine.label_project(depth, code, base, m.min_range, m.max_range, m.floor_tol, m.top, mask, params=m.params, map=m.map, clear=clear, ids=ids,
                                  cells=m.cells if ids else None, pos=m.pos if ids else None)
        return m.cells

    # ------------------------------------------------------------------ ray casts
    def raycast(self, direction=None, origin=None, offsets=None, max_t=1.0, radius=0.0, obstacles="walls", mask=None, into=None):
        """What R rays per env meet first in the env's collision world, by one kernel (mw_ray_cast) with no host value and no
        synchronisation: {"t": float64[N, R], "hit": int32[N, R]} and, with `offsets`, "dir": float64[N, R, 2].

        Ray k of env i is origin + t * direction, t in 0 .. max_t; "t" is the smallest t at which it meets an obstacle and "hit" which
        one — a wall's segment index, engine.RAY_ENT + slot for an entity —, max_t and -1 where it meets none.  With unit directions t
        is metres; with direction = B - A and max_t = 1, t < 1 says that something is in the way from A to B.
        direction  float64[N, R, 2] device tensor of (dx, dz), any length; or
        offsets    float64[R] device tensor of angles in radians added to each agent's heading (a fan; "dir" returns the directions)
        origin     float64[N, R, 3] device tensor (y is not read); None: each env's agent position for all its rays
        radius     0 a ray; > 0 a disc of that radius swept along it (a wall is a capsule, an entity's circle grows by it)
        obstacles  "walls", or "walls+entities": every listed entity but the carried one too
        mask       uint8[N] or bool[N] device tensor: only those envs' rows are read and written
        into       a previous result of the same R (and mode) to write into; without it new tensors are allocated (unmasked rows:
                   t = max_t, hit = -1, dir = 0)
        A NaN in a ray gives max_t and -1; nothing raises on the device.  ValueError for arguments that make no cast; nothing is
        launched then."""
        torch, e = self.torch, self.engine
        n = self.num_envs
        if (direction is None) == (offsets is None):
            raise ValueError("raycast: give exactly one of direction (float64[N, R, 2]) and offsets (float64[R])")
        ok = self._is_tensor
        if offsets is not None:
            if not ok(offsets, (None,)):
                raise ValueError(f"raycast: offsets is a contiguous float64 tensor [R] on {e.device}")
            rays = int(offsets.shape[0])
        else:
            if not ok(direction, (n, None, 2)):
                raise ValueError(f"raycast: direction is a contiguous float64 tensor [{n}, R, 2] on {e.device}")
            rays = int(direction.shape[1])
        if not 1 <= rays <= eng.RAY_MAX:
            raise ValueError(f"raycast: {rays} rays per env outside 1 .. {eng.RAY_MAX}")
        if origin is not None and not ok(origin, (n, rays, 3)):
            raise ValueError(f"raycast: origin is a contiguous float64 tensor [{n}, {rays}, 3] on {e.device}")
        max_t, radius = real("raycast", "max_t", max_t), real("raycast", "radius", radius, lo_open=False)
        flags = self._obstacle_flags("raycast", obstacles)
        mask = self._device_mask(mask, "raycast")
        # the result's tensors: name -> (dtype, shape, what an unmasked row holds)
        want = {"t": (torch.float64, (n, rays), max_t), "hit": (torch.int32, (n, rays), -1)}
        if offsets is not None:
            want["dir"] = (torch.float64, (n, rays, 2), 0.0)
        keys = tuple(want)
        if into is not None:
            if not isinstance(into, dict) or set(into) != set(keys):
                raise ValueError(f"raycast: `into` is a previous result with the keys {keys}")
            for k, (dtype, shape, _) in want.items():
                if not ok(into[k], shape, dtype):
                    raise ValueError(f"raycast: into[{k!r}] is a contiguous {dtype} tensor {list(shape)} on {e.device}")
        out = into or {k: torch.full(shape, fill, dtype=dtype, device=e.device) for k, (dtype, shape, fill) in want.items()}
        params = eng.MwRayParams(max_t, radius, rays, flags)
        e.ray_cast(params, out["t"], out["hit"], out.get("dir"), mask, origin, direction, offsets)
        return out

    def lidar(self, rays=64, fov=2 * math.pi, max_range=10.0, radius=0.0, obstacles="walls+entities"):
        """A range sensor: `rays` distances in a fan around each agent's heading, by one kernel — raycast() with evenly spaced
        offsets, built once per (rays, fov) and kept on the device, unit directions and max_t = max_range.  Returns {"t":
        float64[N, rays], the range in metres (max_range where nothing is hit); "hit": int32[N, rays]; "dir": float64[N, rays, 2], the
        rays' unit directions (x, z), so that agent_pos + t * dir is the point hit}; the tensors are this env's own, reused between
        calls of the same (rays, fov).

        For fov < 2 pi offset k = -fov / 2 + k * fov / (rays - 1) (a single ray looks straight ahead); for the full circle offset
        k = k * 2 pi / rays.  A positive offset turns the ray the way `turn_left` turns the agent: the heading grows, and the agent
        looks along (cos dir, -sin dir) in (x, z) — ray 0 of a fov < 2 pi is the rightmost one, the last the leftmost."""
        torch, e = self.torch, self.engine
        rays, fov = integer("lidar", "rays", rays, 1, eng.RAY_MAX), real("lidar", "fov", fov, hi=2 * math.pi)
        key = (rays, fov)
        if key not in self._lidar_bufs:
            if fov < 2 * math.pi:
                off = [0.0] if rays == 1 else [-fov / 2 + k * fov / (rays - 1) for k in range(rays)]
            else:
                off = [k * 2 * math.pi / rays for k in range(rays)]
            self._lidar_bufs[key] = [torch.tensor(off, dtype=torch.float64, device=e.device), None]
        buf = self._lidar_bufs[key]
        buf[1] = self.raycast(offsets=buf[0], max_t=max_range, radius=radius, obstacles=obstacles, into=buf[1])
        return buf[1]

    # ------------------------------------------------------------------ grid ray casts
    def grid_raycast(self, opaque, direction=None, origin=None, offsets=None, heading=None, max_t=1.0, like=None, cell=0.25, mask=None, into=None):
        """raycast() on the caller's OWN map: what R rays per env meet first among the opaque cells of a grid, by one kernel
        (mw_grid_ray_cast) with no host value and no synchronisation: {"t": float64[N, R], "hit": int32[N, R], "dir": float64[N, R, 2]}.

        Ray k of env i is origin + t * direction, t in 0 .. max_t; "t" is the parameter at which it enters the first opaque cell — 0
        when it starts in one —, "hit" that cell's flat index row * gx + column; max_t and -1 where it meets none.  With unit
        directions t is metres; with direction = B - A and max_t = 1, hit == -1 says that the way from A to B is free on this map.
        opaque     uint8 or bool [N, gz, gx] device tensor: != 0 a cell that stops a ray (a DepthMap's or ScanMap's obstacle plane made
                   contiguous, grid_clearance's inflated plane for a disc, the caller's own raster).  Cells outside the grid stop nothing
        direction  float64[N, R, 2] device tensor of (dx, dz), any length; or
        offsets    float64[R] device tensor of angles in radians added to a heading (raycast()'s fan), with
        heading    float64[N] device tensor, a pose estimate's heading per env; None: each agent's own
        origin     float64[N, R, 3] device tensor (y is not read); None: each env's agent position for all its rays
        like       a NavField, SeenMap, DepthMap, ObjectMap, ScanMap or ScanEvidence whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell`
                   metres per cell as in nav_field()
        mask       uint8[N] or bool[N] device tensor: only those envs' rows are read and written
        into       a previous result of the same R to write into; without it new tensors are allocated (unmasked rows: t = max_t,
                   hit = -1, dir = 0)
        "dir" holds the directions used, so that the result is a `scan` of scan_map_update() and scan_match() as a lidar() one is.  The
        rule in full: include/mwengine.h, "grid ray casts"; a NaN in a ray gives max_t and -1.  The tensors are checked and never
        converted.  ValueError for arguments that make no cast; nothing is launched then."""
        torch, e, n, ok = self.torch, self.engine, self.num_envs, self._is_tensor
        params = self._map_grid("grid_raycast", cell, like, (NavField, SeenMap, DepthMap, ObjectMap, ScanMap, ScanEvidence), "its own")
        if (direction is None) == (offsets is None):
            raise ValueError("grid_raycast: give exactly one of direction (float64[N, R, 2]) and offsets (float64[R])")
        if offsets is not None:
            if not ok(offsets, (None,)):
                raise ValueError(f"grid_raycast: offsets is a contiguous float64 tensor [R] on {e.device}")
            rays = int(offsets.shape[0])
            if heading is not None and not ok(heading, (n,)):
                raise ValueError(f"grid_raycast: heading is a contiguous float64 tensor [{n}] on {e.device}")
        else:
            if heading is not None:
                raise ValueError("grid_raycast: heading without offsets: a heading turns the fan")
            if not ok(direction, (n, None, 2)):
                raise ValueError(f"grid_raycast: direction is a contiguous float64 tensor [{n}, R, 2] on {e.device}")
            rays = int(direction.shape[1])
        if not 1 <= rays <= eng.RAY_MAX:
            raise ValueError(f"grid_raycast: {rays} rays per env outside 1 .. {eng.RAY_MAX}")
        if origin is not None and not ok(origin, (n, rays, 3)):
            raise ValueError(f"grid_raycast: origin is a contiguous float64 tensor [{n}, {rays}, 3] on {e.device}")
        max_t = real("grid_raycast", "max_t", max_t)
        opaque = self._cell_grid("grid_raycast", "opaque", opaque, params.gz, params.gx, optional=False)
        mask = self._device_mask(mask, "grid_raycast")
        want = {"t": (torch.float64, (n, rays), max_t), "hit": (torch.int32, (n, rays), -1), "dir": (torch.float64, (n, rays, 2), 0.0)}
        if into is not None:
            if not isinstance(into, dict) or set(into) != set(want):
                raise ValueError(f"grid_raycast: `into` is a previous result with the keys {tuple(want)}")
            for k, (dtype, shape, _) in want.items():
                if not ok(into[k], shape, dtype):
                    raise ValueError(f"grid_raycast: into[{k!r}] is a contiguous {dtype} tensor {list(shape)} on {e.device}")
        out = into or {k: torch.full(shape, fill, dtype=dtype, device=e.device) for k, (dtype, shape, fill) in want.items()}
        e.grid_ray_cast(params, max_t, rays, opaque, out["t"], out["hit"], out["dir"], mask, origin, direction, offsets, heading)
        return out

    def grid_lidar(self, opaque, rays=64, fov=2 * math.pi, max_range=10.0, heading=None, origin=None, like=None, cell=0.25):
        """The scan a pose would give on the caller's OWN map — lidar() predicted from a map and a pose estimate: grid_raycast() with
        lidar()'s evenly spaced offsets, unit directions and max_t = max_range.  Returns {"t", "hit", "dir"} as lidar() does, "hit" a flat
        cell index; the tensors are this env's own, reused between calls of the same (rays, fov).
        heading  float64[N] device tensor: the estimate's heading; None: each agent's own
        origin   float64[N, 3] device tensor (y is not read): the estimate's position, for all the env's rays; None: each agent's own"""
        torch, e, n = self.torch, self.engine, self.num_envs
        rays, fov = integer("grid_lidar", "rays", rays, 1, eng.RAY_MAX), real("grid_lidar", "fov", fov, hi=2 * math.pi)
        if origin is not None and not self._is_tensor(origin, (n, 3)):
            raise ValueError(f"grid_lidar: origin is a contiguous float64 tensor [{n}, 3] on {e.device}")
        key = (rays, fov, "grid")       # (lidar()'s offsets, in a slot of its own: offsets, the result, the origin per ray)
        if key not in self._lidar_bufs:
            if fov < 2 * math.pi:
                off = [0.0] if rays == 1 else [-fov / 2 + k * fov / (rays - 1) for k in range(rays)]
            else:
                off = [k * 2 * math.pi / rays for k in range(rays)]
            self._lidar_bufs[key] = [torch.tensor(off, dtype=torch.float64, device=e.device), None, None]
        buf = self._lidar_bufs[key]
        if origin is not None:
            if buf[2] is None:
                buf[2] = torch.empty((n, rays, 3), dtype=torch.float64, device=e.device)
            buf[2].copy_(origin[:, None, :].expand(-1, rays, -1))      # (one copy kernel into a kept buffer: no allocation per call)
        buf[1] = self.grid_raycast(opaque, origin=buf[2] if origin is not None else None, offsets=buf[0], heading=heading, max_t=max_range, like=like, cell=cell,
                                   into=buf[1])
        return buf[1]

    # ------------------------------------------------------------------ grid rollouts
    def grid_rollout(self, blocked, plans, field=None, extra=None, pose=None, step=None, radius=None, outside="blocked", stop_at=None, trace=False, like=None,
                     cell=0.25, mask=None, into=None):
        """rollout(render=False, trace=...) on the caller's OWN map: where P candidate plans of T actions per env would take the agent
        on the map it believes in, and what each is worth, by one kernel (mw_grid_plan) with no host value, no synchronisation and no
        env per candidate: a GridRollout.  The inner loop of random shooting, CEM and MPPI for a map-only policy.

        blocked   uint8 or bool [N, gz, gx] device tensor: != 0 an obstacle cell (a ScanMap's or DepthMap's obstacle plane made
                  contiguous).  A move is refused when a disc of `radius` around the new position touches one, or lies in one
        plans     int32 or uint8 [T, N, P] device tensor of actions, time-major as rollout()'s: 0 / 1 turn left / right, 2 / 3 move
                  forward / back, anything else leaves the pose as it is
        field     a NavField — its grid is the call's, as `like=` elsewhere; pass no like or cell then — or a uint16[N, gz, gx] device
                  tensor: `reach` is the least of its values along the plan
        extra     the same kind of tensor as `blocked`: a cost 0 .. 255 summed over the poses behind every step (grid_clearance's cost)
        pose      float64[N, 3] device tensor of (x, z, dir), a pose estimate per env; None: each agent's own
        step      float64[N, 3] device tensor of (forward, drift, turn in degrees) per env; None: the config's defaults
        radius    metres, at most engine.GPLAN_MAX_RADIUS cells; None: the engine's agent_radius; 0: the cell test alone, for a plane
                  that is inflated already
        outside   "blocked": cells outside the grid are obstacles; "open": they are free
        stop_at   a plan stops as soon as its `reach` is <= this (0: at the field's sources); needs a field.  None: never
        trace     with the pose behind every step
        like      a NavField, SeenMap, DepthMap, ObjectMap, ScanMap or ScanEvidence whose grid (cell, gx, gz) is adopted; pass no cell
                  then.  Else `cell` metres per cell as in nav_field()
        mask      uint8[N] or bool[N] device tensor: only those envs' rows are read and written
        into      a GridRollout of the same T, P and trace to write into; without it new tensors are allocated (unmasked rows: 0)
        Where nothing is in the way the poses are, bit for bit, those of rollout()'s trace.  The rule in full: include/mwengine.h,
        "grid rollouts".  The tensors are checked and never converted.  ValueError for arguments that make no call; nothing is
        launched then."""
        torch, e, n, where = self.torch, self.engine, self.num_envs, "grid_rollout"
        kinds = (NavField, SeenMap, DepthMap, ObjectMap, ScanMap, ScanEvidence)
        if isinstance(field, NavField):
            if like is not None or cell != 0.25:
                raise ValueError(f"{where}: a NavField's grid is the call's: pass no like or cell")
            like = field
        params = self._map_grid(where, cell, like, kinds, "its own")
        if isinstance(field, NavField):
            field = field.field
        if field is not None and not self._is_tensor(field, (n, params.gz, params.gx), torch.uint16):
            raise ValueError(f"{where}: field is a NavField or a contiguous uint16 tensor [{n}, {params.gz}, {params.gx}] on {e.device}")
        if not any(self._is_tensor(plans, (None, n, None), dt) for dt in (torch.int32, torch.uint8)):
            raise ValueError(f"{where}: plans is a contiguous int32 or uint8 tensor [T, {n}, P] on {e.device}")
        T, P = int(plans.shape[0]), int(plans.shape[2])
        if not 1 <= T <= eng.MAX_PLAN:
            raise ValueError(f"{where}: T = {T} outside 1 .. {eng.MAX_PLAN}")
        if not 1 <= P <= eng.GPLAN_MAX_PLANS:
            raise ValueError(f"{where}: {P} plans per env outside 1 .. {eng.GPLAN_MAX_PLANS}")
        for name, t in (("pose", pose), ("step", step)):
            if t is not None and not self._is_tensor(t, (n, 3)):
                raise ValueError(f"{where}: {name} is a contiguous float64 tensor [{n}, 3] on {e.device}")
        radius = float(e.cfg.agent_radius) if radius is None else real(where, "radius", radius, lo_open=False)
        if radius > eng.GPLAN_MAX_RADIUS * params.cell:
            raise ValueError(f"{where}: radius {radius!r} is more than {eng.GPLAN_MAX_RADIUS} cells of {params.cell!r}")
        if outside not in ("blocked", "open"):
            raise ValueError(f"{where}: outside {outside!r}; have 'blocked' and 'open'")
        if stop_at is not None:
            stop_at = integer(where, "stop_at", stop_at, 0, 0xFFFF)
            if field is None:
                raise ValueError(f"{where}: stop_at without a field: there is nothing to reach")
        if not isinstance(trace, bool):
            raise ValueError(f"{where}: trace must be True or False, not {trace!r}")
        blocked = self._cell_grid(where, "blocked", blocked, params.gz, params.gx, optional=False)
        extra = self._cell_grid(where, "extra", extra, params.gz, params.gx)
        mask = self._device_mask(mask, where)
        if into is not None:
            if not isinstance(into, GridRollout):
                raise ValueError(f"{where}: `into` must be a GridRollout")
            if (not self._is_tensor(into.pose, (n, P, 3)) or not self._is_tensor(into.stats, (n, P, 5), torch.int32)
                    or (into.trace is not None) != trace or (trace and not self._is_tensor(into.trace, (T, n, P, 3)))):
                raise ValueError(f"{where}: `into` is a GridRollout of T = {T}, P = {P} and trace = {trace} on {e.device}")
            out = into
        else:
            out = GridRollout(torch.zeros((n, P, 3), dtype=torch.float64, device=e.device), torch.zeros((n, P, 5), dtype=torch.int32, device=e.device),
                              torch.zeros((T, n, P, 3), dtype=torch.float64, device=e.device) if trace else None, params)
        e.grid_plan(params, radius, eng.GPLAN_OUTSIDE_BLOCKS if outside == "blocked" else 0, -1 if stop_at is None else stop_at, blocked, plans, out.pose, out.stats,
                    out.trace, field, extra, pose, step, mask)
        return out
