"""The engine's configuration of a family, decided on the host with no torch and no engine object: the table of registered ids
(`_KIND`), the auto-reset modes, and build_config(), which turns a family's template world and the constructor's choices into the
mw_config the engine is created with and the lists of assets to upload.  vec_env.py re-exports the names."""
from __future__ import annotations

import math
from typing import NamedTuple

from . import engine as eng
from .scene import base_config

_KIND = {
    "MiniWorld-Hallway-v0": ("Hallway", eng.GEN_HALLWAY, eng.TASK_GOTO, 3),
    "MiniWorld-OneRoom-v0": ("OneRoom", eng.GEN_ONEROOM, eng.TASK_GOTO, 3),
    "MiniWorld-OneRoomS6-v0": ("OneRoomS6", eng.GEN_ONEROOM, eng.TASK_GOTO, 3),
    "MiniWorld-OneRoomS6Fast-v0": ("OneRoomS6Fast", eng.GEN_ONEROOM, eng.TASK_GOTO, 3),     # S6 + its own step / turn sizes
    "MiniWorld-Maze-v0": ("Maze", eng.GEN_MAZE, eng.TASK_GOTO, 3),
    "MiniWorld-MazeS2-v0": ("MazeS2", eng.GEN_MAZE, eng.TASK_GOTO, 3),
    "MiniWorld-MazeS3-v0": ("MazeS3", eng.GEN_MAZE, eng.TASK_GOTO, 3),
    "MiniWorld-MazeS3Fast-v0": ("MazeS3Fast", eng.GEN_MAZE, eng.TASK_GOTO, 3),
    "MiniWorld-PickupObjects-v0": ("PickupObjects", eng.GEN_PICKUP, eng.TASK_PICKUP, 5),
    # fixed floorplans: _gen_world compiled into a placement program the device generator runs (genprog.py)
    "MiniWorld-FourRooms-v0": ("FourRooms", eng.GEN_PROGRAM, eng.TASK_GOTO, 3),
    "MiniWorld-TMaze-v0": ("TMaze", eng.GEN_PROGRAM, eng.TASK_GOTO, 3),
    "MiniWorld-TMazeLeft-v0": ("TMazeLeft", eng.GEN_PROGRAM, eng.TASK_GOTO, 3),
    "MiniWorld-TMazeRight-v0": ("TMazeRight", eng.GEN_PROGRAM, eng.TASK_GOTO, 3),
    "MiniWorld-YMaze-v0": ("YMaze", eng.GEN_PROGRAM, eng.TASK_GOTO, 3),
    "MiniWorld-YMazeLeft-v0": ("YMazeLeft", eng.GEN_PROGRAM, eng.TASK_GOTO, 3),
    "MiniWorld-YMazeRight-v0": ("YMazeRight", eng.GEN_PROGRAM, eng.TASK_GOTO, 3),
    "MiniWorld-WallGap-v0": ("WallGap", eng.GEN_PROGRAM, eng.TASK_GOTO, 3),
    "MiniWorld-ThreeRooms-v0": ("ThreeRooms", eng.GEN_PROGRAM, eng.TASK_NONE, 3),
    # the forbidden street / the touch table + end-of-episode action are K1 task rules fed by the program's tables
    "MiniWorld-Sidewalk-v0": ("Sidewalk", eng.GEN_PROGRAM, eng.TASK_SIDEWALK, 3),
    "MiniWorld-Sign-v0": ("Sign", eng.GEN_PROGRAM, eng.TASK_SIGN, 4),
    "MiniWorld-PutNext-v0": ("PutNext", eng.GEN_PROGRAM, eng.TASK_PUTNEXT, 8),
    "MiniWorld-RoomObjects-v0": ("RoomObjects", eng.GEN_PROGRAM, eng.TASK_NONE, 8),
    # health bookkeeping and the respawn of a consumed kit (place_entity at the END of the entity list,
    # collecthealth.py:79-98) are a K1 task rule too
    "MiniWorld-CollectHealth-v0": ("CollectHealth", eng.GEN_PROGRAM, eng.TASK_COLLECT, 8),
}


AUTORESET_MODES = {True: "same_step", False: "off", "same_step": "same_step", "next_step": "next_step", "levels": "levels", "seeds": "seeds"}
_ENGINE_AUTORESET = {"same_step": eng.AUTORESET_SAME_STEP, "next_step": eng.AUTORESET_NEXT_STEP, "off": eng.AUTORESET_OFF,
                     "levels": eng.AUTORESET_OFF,       # (levels: the loads behind the step restart the envs)
                     "seeds": eng.AUTORESET_SAME_STEP}
_INFO_KIND = {"CollectHealth": "health", "TMaze": "goal_pos", "TMazeLeft": "goal_pos", "TMazeRight": "goal_pos",
              "YMaze": "goal_pos", "YMazeLeft": "goal_pos", "YMazeRight": "goal_pos"}


class EnvConfig(NamedTuple):
    """What build_config() decides: the mw_config the engine is created with, the resident texture names in id order, whether they
    are domain-randomisation variants (beyond the template scene's own), and the mesh names to upload ahead of the scene's."""
    cfg: eng.MwConfig
    textures: list
    tex_dr: bool
    meshes: list


def _ball_key_meshes():
    """all 12 ball / key meshes: ids ball_<colour> = 0..5, key_<colour> = 6..11 in sorted colour order"""
    from .entity import COLOR_NAMES
    return [f"ball_{c}" for c in COLOR_NAMES] + [f"key_{c}" for c in COLOR_NAMES]


def _entity_slots(template):
    """the template's entities in slot order (the agent has none)"""
    return [e for e in template.entities if e is not template.agent]


def _fill(array, values):
    for i, v in enumerate(values):
        array[i] = float(v)


def _room_args(cfg, template, sc):
    """GEN_HALLWAY / GEN_ONEROOM: the room's extent, where the box and the agent may be, the agent's heading range, the box size"""
    room = template.rooms[0]
    if cfg.generator == eng.GEN_HALLWAY:
        rest = [room.max_x - 2, room.max_x - 2, math.pi / 4, 0.8]
    else:
        rest = [room.min_x, room.max_x, math.pi, 0.8]
    _fill(cfg.gen_args, [room.min_x, room.max_x, room.min_z, room.max_z] + rest)


def _maze_tables(cfg, template, sc):
    """GEN_MAZE: rows, columns, room and gap size, wall height, the three texture ids; TEX_DENSITY / size of each texture"""
    r0 = template.rooms[0]
    texs = [r0.floor_tex, r0.ceil_tex, r0.wall_tex]
    names = [str(v) for v in sc["tex_names"]]
    _fill(cfg.gen_tab, [template.num_rows, template.num_cols, template.room_size, template.gap_size, r0.wall_height]
          + [names.index(x.variant) for x in texs])
    _fill(cfg.gen_colors, [512 / d for x in texs for d in (x.width, x.height)])


def _pickup_tables(cfg, template, sc):
    """GEN_PICKUP: the room, per kind (Ball, Box, Key) radius, height, scale and first mesh id, and the six colours' RGB"""
    from .entity import COLOR_NAMES, COLORS, Ball, Box, Key
    room = template.rooms[0]
    _fill(cfg.gen_args, [room.min_x, room.max_x, room.min_z, room.max_z])
    protos = (Ball(COLOR_NAMES[0], size=0.9), Box(COLOR_NAMES[0], size=0.9), Key(COLOR_NAMES[0]))
    _fill(cfg.gen_tab, [v for proto, first_mesh in zip(protos, (0, -1, 6))
                        for v in (proto.radius, proto.height, getattr(proto, "scale", 1.0), first_mesh)])
    _fill(cfg.gen_colors, [COLORS[c][j] for c in COLOR_NAMES for j in range(3)])


_GENERATOR_TABLES = {eng.GEN_HALLWAY: _room_args, eng.GEN_ONEROOM: _room_args, eng.GEN_MAZE: _maze_tables, eng.GEN_PICKUP: _pickup_tables}


def _room_variants(cfg, template, sc):
    """Texture domain randomisation of a generated single-room world: the variant tables of its wall, floor and ceiling (ids,
    TEX_DENSITY / size) and the room's shape go into cfg; returns the resident names, or None when no slot has a choice."""
    from . import assets
    room0 = template.rooms[0]
    variants = [assets.texture_variants(t) for t in (room0.wall_tex_name, room0.floor_tex_name, room0.ceil_tex_name)]
    if not any(len(v) > 1 for v in variants):
        return None
    names = [str(v) for v in sc["tex_names"]]
    for k, vs in enumerate(variants):
        cfg.tex_nvar[k] = len(vs)
        for j, v in enumerate(vs):
            if v not in names:
                names.append(v)
            cfg.tex_var_id[k][j] = names.index(v)
            w, h = assets.texture_size(v)
            cfg.tex_var_scale[k][j][0], cfg.tex_var_scale[k][j][1] = 512 / w, 512 / h
    cfg.room_wall_height = float(room0.wall_height)
    cfg.room_no_ceiling = int(bool(room0.no_ceiling))
    return names


def _program_variants(template, sc):
    """Texture domain randomisation of a placement program, whose rooms may each name their own textures: every variant of every room
    texture is resident (the program's tables name them); returns the names, or None when no texture has a choice."""
    from . import assets
    room_names = sorted({n for r in template.rooms for n in (r.wall_tex_name, r.floor_tex_name, r.ceil_tex_name)})
    if not any(len(assets.texture_variants(n)) > 1 for n in room_names):
        return None
    names = [str(v) for v in sc["tex_names"]]
    for n in room_names:
        names += [v for v in assets.texture_variants(n) if v not in names]
    return names


def build_config(env_id, template, sc, num_envs, device_id=0, domain_rand=False, msaa=8, autoreset_mode="same_step", rng="auto"):
    """The engine configuration of a family: `template` is its host world after reset(seed), `sc` that world's scene
    (scene_from_env), the rest the constructor's choices.  Returns an EnvConfig; nothing is uploaded or created here."""
    cls_name, generator, task, _ = _KIND[env_id]
    P, S, E = len(sc["polys_nv"]), len(sc["wall_segs"]), max(1, len(sc["ents_kind"]))
    if cls_name == "PickupObjects":
        E = max(E, template.num_objs)
    cfg = base_config(num_envs, template.obs_width, template.obs_height, E, P, S,
                      max_visible=-(-(P + 6 * E) // 16) * 16,
                      params_ranges=template.params.as_ranges(), device_id=device_id)
    cfg.msaa = int(msaa)
    cfg.task, cfg.goal_ent, cfg.num_objs = task, 0, len(sc["ents_kind"])
    ents = _entity_slots(template)
    if task in (eng.TASK_GOTO, eng.TASK_SIDEWALK) and hasattr(template, "box"):
        cfg.goal_ent = ents.index(template.box)
    if task == eng.TASK_PUTNEXT:
        cfg.goal_ent, cfg.goal_ent2 = ents.index(template.red_box), ents.index(template.yellow_box)
    cfg.max_episode_steps = int(min(float(template.max_episode_steps), 2 ** 30))
    cfg.domain_rand = int(domain_rand)
    cfg.generator = generator
    cfg.autoreset = _ENGINE_AUTORESET[autoreset_mode]
    cfg.agent_radius = float(template.agent.radius)
    cfg.rng_mode = eng.RNG_PHILOX if rng == "philox" else eng.RNG_PCG64     # (every device generator draws numpy's PCG64 stream)
    if generator in _GENERATOR_TABLES:
        _GENERATOR_TABLES[generator](cfg, template, sc)
    # texture domain randomisation needs one geometry set per env (texcoords depend on the variant)
    variants = None
    if domain_rand:
        variants = _program_variants(template, sc) if generator == eng.GEN_PROGRAM else _room_variants(cfg, template, sc)
    cfg.shared_geometry = int(generator != eng.GEN_MAZE and variants is None)
    # PickupObjects, RoomObjects: any mix of kinds and colours can be generated on the device, so all twelve meshes are resident
    meshes = _ball_key_meshes() if cls_name in ("PickupObjects", "RoomObjects") else []
    return EnvConfig(cfg, variants or [str(v) for v in sc["tex_names"]], variants is not None, meshes)
