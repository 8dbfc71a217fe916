"""Synthetic scenes that put a frame ON the raster kernels' capacity limits (plain numpy: no GPU, no engine).

A scene is the neutral scene dict of oracle/pyoracle.py.  Each `*_world` below returns ONE polygon set — the engine's test
glue shares a batch's geometry between its envs — and the poses that look at its parts:

    world, poses, parts = crowded_world(base)  # poses: name -> the scene keys a pose changes; parts: name -> its polygons
    scene = posed(world, poses["slats"])

The parts are free-standing quads and triangles in front of a camera: inside the Hallway fixture's room where a limit needs neighbouring
tiles that hold the room only, otherwise at stations out in the open, STATION_GAP metres apart to the side of each other and
beyond the far plane's reach of the room, every camera looking along +x: from a station nothing but its own part is in the
frustum.  Every synthetic polygon has its own colour (every other one is textured as well), so a wrong winner changes pixels.

Sizes are chosen against the 80 x 60 frame at the fixtures' 60 degree field of view: at 1 m a pixel is 0.01925 m, a 16 x 4
tile 0.308 m x 0.077 m, and the view axis runs through the middle of tile (2, 7): columns 32 .. 47, rows 28 .. 31.
"""
import numpy as np

STATION_X = 160.0           # the stations' cameras (the Hallway lies around the origin: more than the far plane's 100 m behind them)
STATION_GAP = 40.0          # sideways (z) between stations: a neighbour's part is 88 degrees off the view axis


def bare(base):
    """The base scene (a fixture frame) with its entities switched off, arrays copied."""
    sc = {k: np.array(v, copy=True) for k, v in base.items()}
    sc["ents_kind"] = np.zeros_like(sc["ents_kind"])
    return sc


def posed(world, pose):
    sc = dict(world)
    for k, v in pose.items():
        sc[k] = np.float64(v) if np.ndim(v) == 0 else np.array(v, np.float64)
    return sc


def view_axes(agent_dir):
    """forward and right of a camera without pitch (oracle/mwo_geom.c: the heading turns about +y)"""
    d = float(agent_dir)
    return np.array([np.cos(d), 0.0, -np.sin(d)]), np.array([np.sin(d), 0.0, np.cos(d)])


UP = np.array([0.0, 1.0, 0.0])
POLY_KEYS = ("polys_v", "polys_uv", "polys_n", "polys_nv", "polys_tex", "polys_rgb", "polys_xf")


def eye_of(scene):
    fwd, _ = view_axes(scene["agent_dir"])
    return np.array(scene["agent_pos"], np.float64) + fwd * float(scene["cam_fwd_disp"]) + UP * float(scene["cam_height"])


def quad(centre, right, up, half_w, half_h):
    """corners of a rectangle that faces a viewer who sees `right` to the right and `up` upwards (counter-clockwise)"""
    return np.array([centre + right * (half_w * u) + up * (half_h * v) for u, v in ((-1, -1), (1, -1), (1, 1), (-1, 1))])


def colours(n, first=0):
    """colours first .. first + n - 1 of a table of 97 distinct ones, none dark, neighbours in the table far apart"""
    assert first + n <= 97
    c = (first + np.arange(n))[:, None] * np.array([[37, 59, 83]]) % 97 / 96.0
    return (0.25 + 0.75 * c).astype(np.float32)


def append_quads(scene, quads, normal, rgb, tex=None):
    """The scene with the polygons drawn after its own: quads n x [4][3] (or [3][3]: triangles), one normal for all, rgb
    [n][3]; every other one carries texture `tex` (an index of scene["tex_names"], default: none is textured)."""
    n = len(quads)
    sc = dict(scene)
    t = np.full(n, -1, np.int32)
    if tex is not None:
        t[::2] = tex
    uv = np.tile(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), (n, 1, 1))
    nv = np.array([len(q) for q in quads], np.int32)
    verts = np.array([np.concatenate([q, q[-1:]]) if len(q) == 3 else q for q in quads], np.float32)
    sc["polys_v"] = np.concatenate([scene["polys_v"], verts])
    sc["polys_uv"] = np.concatenate([scene["polys_uv"], uv])
    sc["polys_n"] = np.concatenate([scene["polys_n"], np.tile(np.asarray(normal, np.float32), (n, 1))])
    sc["polys_nv"] = np.concatenate([scene["polys_nv"], nv])
    sc["polys_tex"] = np.concatenate([scene["polys_tex"], t])
    sc["polys_rgb"] = np.concatenate([scene["polys_rgb"], np.asarray(rgb, np.float32)])
    sc["polys_xf"] = np.concatenate([scene["polys_xf"], np.zeros((n, scene["polys_xf"].shape[1]), np.float32)])
    return sc


# ------------------------------------------------------------------ the parts (eye, forward, right -> quads)

def slats(eye, fwd, right, n, pitch=0.007, half_w=0.0025, half_h=0.03, dist=1.0):
    """n thin upright quads side by side, facing the camera, all inside the tile the view axis runs through"""
    return [quad(eye + fwd * dist + right * ((j - (n - 1) / 2) * pitch), right, UP, half_w, half_h) for j in range(n)]


def slivers(eye, fwd, right, n, **kw):
    """the slats as triangles (base below, tip above): ONE list entry per primitive — more than 16 of them on a tile in a
    list that still fits the quad kernel's staged records"""
    return [np.stack([q[0], q[1], 0.5 * (q[2] + q[3])]) for q in slats(eye, fwd, right, n, **kw)]


def interleaved_slats(eye, fwd, right, n=7, half_w=0.02, half_h=0.25, dist=1.0, step=0.02):
    """neighbours overlap by a third of their width, every other one `step` further away: no triangle covers a quad that
    its neighbour touches everywhere, samples are contested along every seam"""
    pitch = 2 * half_w * 2 / 3
    return [quad(eye + fwd * (dist + step * (j & 1)) + right * ((j - (n - 1) / 2) * pitch), right, UP, half_w, half_h) for j in range(n)]


def crossing_pair(eye, fwd, right, half=0.3, dist=1.0, tilt=0.02):
    """two quads that interpenetrate along a diagonal of the frame: one leans back to the right and up, the other to the left
    and down by `tilt` radians — the depth order flips inside the pixels of the seam"""
    out = []
    for s in (1.0, -1.0):
        r = right * np.cos(s * tilt) + fwd * np.sin(s * tilt)
        u = UP * np.cos(s * tilt) + fwd * np.sin(s * tilt)
        out.append(quad(eye + fwd * dist, r, u, half, half))
    return out


def coplanar_twins(eye, fwd, right, half=0.2, dist=1.0):
    """the same quad twice (GL_LESS: the one drawn first wins everywhere)"""
    q = quad(eye + fwd * dist, right, UP, half, half)
    return [q, q.copy()]


def layers(eye, fwd, right, k, dist=1.0, step=0.05):
    """k parallel quads, each covering the whole frame, the nearest drawn LAST"""
    return [quad(eye + fwd * (dist + step * (k - 1 - j)), right, UP, 2.0, 2.0) for j in range(k)]


def fence(eye, fwd, right, k, size=0.08, gap=0.12, dist=1.5):
    """k small separated quads on a line across the view: a heading decides how many of them are in the frustum"""
    return [quad(eye + fwd * dist + right * ((j - (k - 1) / 2) * gap), right, UP, size / 2, size / 2) for j in range(k)]


# ------------------------------------------------------------------ worlds

def _station(k):
    """pose of the k-th station: out in the open, looking along +x"""
    return {"agent_pos": [STATION_X, 0.0, STATION_GAP * k], "agent_dir": 0.0, "cam_pitch": 0.0}


LAYER_COUNTS = (1, 2, 3, 4, 5)
N_SLIVERS = 22
N_MESH_SLIVERS = 18         # with the PickupObjects fixture's room and boxes: a list of 37


def _world(base, tex, items):
    """the room and the parts `items` [(name, pose, eye, forward, right -> polygons)]: (world, poses, parts) — parts: name ->
    slice of the world's polygons"""
    room = bare(base)
    room["cam_pitch"] = np.float64(0.0)
    world, poses, parts, used = room, {}, {}, 0
    for name, pose, make in items:
        sc = posed(room, pose)
        fwd, right = view_axes(sc["agent_dir"])
        quads = make(eye_of(sc), fwd, right)
        first = len(world["polys_nv"])
        world = append_quads(world, quads, -fwd, colours(len(quads), used), tex)
        poses[name], parts[name] = pose, slice(first, first + len(quads))
        used += len(quads)
    assert len(world["polys_nv"]) <= 64     # (worlds of more polygons have their hidden ones culled before the list: other lengths)
    return world, poses, parts


def crowded_world(base, tex=None):
    """The room with 24 slats in front of the base frame's camera ("slats": one tile with far more than 16 triangles between
    tiles that hold the room only, in a list longer than the quad kernel stages) and 22 slivers behind it ("slivers": the same
    in a list that it does stage), and a station with 8 slats and nothing else ("slats16": 16 triangles on one tile, no more)."""
    here = {"agent_pos": np.array(base["agent_pos"], np.float64), "agent_dir": float(base["agent_dir"]), "cam_pitch": 0.0}
    back = dict(here, agent_dir=here["agent_dir"] + np.pi)          # from the same spot, the other way: each part behind the other's camera
    return _world(base, tex, [("slats", here, lambda e, f, r: slats(e, f, r, 24)),
                              ("slivers", back, lambda e, f, r: slivers(e, f, r, N_SLIVERS)),
                              ("slats16", _station(0), lambda e, f, r: slats(e, f, r, 8))])


def overlap_world(base, tex=None):
    """Stations with interleaved slats, the crossing pair, the coplanar twins, 1 .. 5 layers, and 8 slats with a sliver beside
    them ("slats17": 17 triangles on one tile, the first count past its 16 slots).  The room is part of the world, no station
    sees it."""
    items = [("interleaved", _station(0), interleaved_slats), ("crossing", _station(1), crossing_pair), ("twins", _station(2), coplanar_twins)]
    items += [(f"layers{k}", _station(2 + k), lambda e, f, r, k=k: layers(e, f, r, k)) for k in LAYER_COUNTS]
    items.append(("slats17", _station(3 + len(LAYER_COUNTS)), lambda e, f, r: slats(e, f, r, 9)[:8] + slivers(e, f, r, 9)[8:]))
    return _world(base, tex, items)


FILLING_PARTS = ("cover", "upper", "lower", "right", "left", "floor")


def frame_filling_world(base, aspect=80 / 60, tex=None):
    """Stations whose polygons reach past the frustum, so that clipping leaves their vertices ON the frame's borders and corners: the
    edges with the largest slopes a frame of `aspect` = W / H can hold (a full-width edge has dcdy = +-256 W, a full-height one dcdx =
    +-256 H, the diagonals both; miniworld_amd/csrc/mw_edge_rec.h).
      cover   a quad three times the frustum at 1 m, its sides in the frame's proportion: clipped, its two triangles meet along the
              frame's diagonal and their other edges are the frame's borders, each in one direction
      upper, lower   the halves of the same quad above and below the diagonal from bottom left to top right, one alone per station
      right, left    the halves beside the other diagonal: every corner-to-corner edge is drawn in both windings
      floor   a wide horizontal quad below the eye that the bottom, left and right planes clip, and its mirror image above as ceiling
    The room is part of the world, no station sees it."""
    ty = np.tan(np.radians(float(base["cam_fov_y"])) / 2.0)
    tx = ty * aspect

    def corners(e, f, r):
        return quad(e + f * 1.0, r, UP, 3.0 * tx, 3.0 * ty)          # bottom left, bottom right, top right, top left

    def level(e, f, r):
        # 0.2 .. 3.2 m ahead, 8 m to each side (past the side planes of a 128 x 48 frame there, 84 degrees off a neighbour's axis), 0.5 m below / above the eye
        return [quad(e + f * 1.7 - UP * 0.5, r, f, 8.0, 1.5), quad(e + f * 1.7 + UP * 0.5, r, -f, 8.0, 1.5)]
    halves = {"upper": (0, 2, 3), "lower": (0, 1, 2), "right": (1, 2, 3), "left": (0, 1, 3)}
    items = [("cover", _station(0), lambda e, f, r: [corners(e, f, r)])]
    items += [(name, _station(1 + k), lambda e, f, r, ids=ids: [corners(e, f, r)[list(ids)]]) for k, (name, ids) in enumerate(halves.items())]
    items.append(("floor", _station(1 + len(halves)), level))
    assert tuple(name for name, _, _ in items) == FILLING_PARTS
    return _world(base, tex, items)


def only(world, part):
    """the world's polygons of one part alone (a slice of them)"""
    sc = dict(world)
    for k in POLY_KEYS:
        sc[k] = world[k][part]
    return sc


FENCE_ROOM, FENCE_OPEN = 40, 16


def fence_world(base, tex=None):
    """The room with a fence of 40 quads across the view of the base frame's camera, and a station with a fence of 16 and
    nothing else.  Returns (world, {"room": pose, "open": pose}): a length-sweep pose is one of the two with its own
    agent_dir (and cam_pitch)."""
    room = bare(base)
    room["cam_pitch"] = np.float64(0.0)
    here = {"agent_pos": np.array(room["agent_pos"], np.float64), "agent_dir": float(room["agent_dir"]), "cam_pitch": 0.0}
    there = _station(0)
    world = room
    for k, (pose, n, gap) in enumerate(((here, FENCE_ROOM, 0.11), (there, FENCE_OPEN, 0.12))):
        sc = posed(room, pose)
        fwd, right = view_axes(sc["agent_dir"])
        world = append_quads(world, fence(eye_of(sc), fwd, right, n, gap=gap), -fwd, colours(n, FENCE_ROOM * k), tex)
    return world, {"room": here, "open": there}


SLATS_RAISED = 12 * 0.01925     # 12 pixels above the view axis at 1 m: the middle of tile row 4 (rows 16 .. 19), above the horizon


def mesh_world(base, tex=None):
    """A fixture frame WITH its entities (meshes on the floor, below the horizon of a camera without pitch) and 18 slivers
    above the horizon: the slivers' tile lies outside every mesh's tile rectangle.  Returns (world, pose, part)."""
    world = {k: np.array(v, copy=True) for k, v in base.items()}
    world["cam_pitch"] = np.float64(0.0)
    fwd, right = view_axes(world["agent_dir"])
    first = len(world["polys_nv"])
    quads = slivers(eye_of(world) + UP * SLATS_RAISED, fwd, right, N_MESH_SLIVERS)
    world = append_quads(world, quads, -fwd, colours(N_MESH_SLIVERS), tex)
    pose = {"agent_pos": np.array(world["agent_pos"], np.float64), "agent_dir": float(world["agent_dir"]), "cam_pitch": 0.0}
    return world, pose, slice(first, first + N_MESH_SLIVERS)
