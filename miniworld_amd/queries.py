"""The world queries of the batched env — navigation fields, explored-area maps, grid sight, grid regions, egocentric map windows, depth projection,
label frames, object maps, ray casts —, each one kernel on the device with no host value: their value classes (NavField, SeenMap, EgoWindow,
DepthWindow, DepthMap, LabelFrame, ObjectWindow, ObjectMap, GridRegions) and
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
            cell, gx, gz = like.cell, like.gx, like.gz
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
        like      a NavField, SeenMap, DepthMap or ObjectMap whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell` metres
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
            g = self._map_grid("grid_field", cell, like, (NavField, SeenMap, DepthMap, ObjectMap), "its own")
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
        like       a NavField, SeenMap, DepthMap or ObjectMap whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell`
                   metres per cell as in nav_field()
        mask       uint8[N] or bool[N] device tensor: only those envs' rows are computed (the others are neither read nor written)
        seen       uint8 or bool [N, gz, gx] device tensor: every cell any viewpoint of the env sees is set to 1; never cleared here
        A cell is seen when its centre is within max_range and the cone of the viewpoint's centre and no opaque cell's closed square
        meets the segment between the two (include/mwengine.h, "grid sight"): a viewpoint sees itself, and an opaque cell's face.
        The tensors are checked and never converted.  ValueError for arguments that make no call; nothing is launched then."""
        torch, e = self.torch, self.engine
        params = self._map_grid("grid_sight", cell, like, (NavField, SeenMap, DepthMap, ObjectMap), "its own")
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
        like          a NavField, SeenMap, DepthMap or ObjectMap whose grid (cell, gx, gz) is adopted; pass no cell then.  Else `cell`
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
            params = self._map_grid("grid_regions", cell, like, (NavField, SeenMap, DepthMap, ObjectMap), "its own")
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
        like        a NavField, SeenMap or ObjectMap whose grid (cell, gx, gz) the map adopts, so that they line up cell for cell; pass no
                    cell then
        min_points  how many pixels of ONE depth map must fall into a cell to set it, 1 .. 255
        min_range, max_range, floor_tol, top  as for depth_window()
        At most 16384 cells (the kernel counts in 64 KiB of LDS): ValueError says "use a larger cell" otherwise."""
        torch, e = self.torch, self.engine
        params = self._map_grid("depth_map", cell, like, (NavField, SeenMap, ObjectMap), "its own")
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
        like   a NavField, SeenMap, DepthMap or ObjectMap whose grid (cell, gx, gz) the map adopts, so that they line up cell for cell; pass
               no cell then
        ids    K, 0 .. 255: `cells` and `pos` have a row for each id below it (an id from K on is mapped, not counted); None: the env's
               entity slots, at most 255.  0: the map alone
        min_range, max_range, floor_tol, top  as for depth_window()
        At most 16384 cells (the kernel keeps a key per cell in LDS): ValueError says "use a larger cell" otherwise."""
        torch, e = self.torch, self.engine
        params = self._map_grid("object_map", cell, like, (NavField, SeenMap, DepthMap, ObjectMap), "its own")
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

