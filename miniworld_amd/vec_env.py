"""MiniWorldVecEnv — N environments stepped and rendered in lockstep on one MI355X.

This is the performance path: world state lives on the device as Structure-of-Arrays, one
``step()`` is three kernel launches (step, geometry, raster; two more with mesh entities) that write the
``uint8[N,60,80,3]`` observation tensor (and optionally ``float32[N,60,80,1]`` depth) straight into torch memory.
Episodes auto-reset on the device.  ``autoreset=True`` / ``"same_step"`` (the default): the observation returned together
with ``terminated|truncated`` is the first one of the next episode.  ``autoreset="next_step"``: the step that ends an
episode returns its terminal frame, reward and flags, and the env's next step ignores its action and returns the next
episode's first frame with reward 0 and no flags — the reference's own "step; if done: reset()" (it leaves the reset to the
caller, scripts/benchmark.py:36-37), on the same random stream.  ``autoreset=False``: the caller resets.
``autoreset="levels"``: a finished env restarts, in the same step and without the host learning that it finished, from a
record of a bank of levels the caller chose (``make_levels``, ``set_levels``, ``next_level``).
``autoreset="seeds"``: the same-step auto-reset from seeds the device holds — a finished env starts, in the same step, the episode
of ``env.reset(seed=next_seed[i])``; ``next_seed`` (int64[N] on the device) is the caller's to write between steps, ``episode_seed``
tells which seed each env is playing.  Eight bytes per level, no bank to build, any seed.

All 23 env ids are generated, ruled and auto-reset on the device, on the reference's own numpy PCG64 stream: Hallway,
OneRoom*, Maze* and PickupObjects through their own generators, the fixed-floorplan families through placement programs
(`genprog.py`).  `host_generate()` (the host world generator + `mw_set_state`) remains as an injection API.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import engine as eng
from . import envs as _envs
from .scene import base_config, polys_array, scene_from_env, state_arrays, upload_scene_meshes

class NavField:
    """A navigation field (MiniWorldVecEnv.nav_field): `field`, the uint16[N, gz, gx] device tensor of shortest-path costs — 0xFFFF a
    blocked cell, 0xFFFE one no path reaches, a move costs 5 straight and 7 diagonally —, the grid (`cell` metres per cell, gx x gz
    cells from the env's own min_x, min_z), and what it leads to: `target`, an entity slot or a float64[N, 3] device tensor.  The
    tensor is the caller's, like a level bank: the engine keeps nothing of it."""

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


# ------------------------------------------------------------------ the engine's configuration (no torch, no engine)

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


class EnvSnapshot:
    """Records of MiniWorldVecEnv.save_state(): `data`, the engine's opaque uint8 record buffer (a torch tensor; its header carries
    the layout key of the configuration it was taken under), `count`, the valid records, and `capacity`, the records the buffer was
    laid out for.  A snapshot taken with frames=True also holds `frames`, the engine's frame record buffer (the observation, depth
    and stacked frames each env had at the save), `frame_flags`, the engine.SNAPF_* bits it was saved under, and `frame_stack`, the
    stack depth K of its stacks (0: none); without frames they are None, 0 and 0.  `.cpu()` / `.to(device)` move it, so
    `torch.save(snap.cpu().state_dict(), path)` and `EnvSnapshot.from_state_dict(torch.load(path))` write a checkpoint and read it
    back.  A bank of levels (MiniWorldVecEnv.make_levels) also carries `seeds`, the int64 tensor of the seed each record was reset
    with; None otherwise."""

    def __init__(self, data, count: int, capacity: int, frames=None, frame_flags: int = 0, frame_stack: int = 0, seeds=None):
        self.data, self.count, self.capacity = data, int(count), int(capacity)
        self.frames = frames
        self.frame_flags, self.frame_stack = (int(frame_flags), int(frame_stack)) if frames is not None else (0, 0)
        self.seeds = seeds

    def _with(self, move):
        return EnvSnapshot(move(self.data), self.count, self.capacity, None if self.frames is None else move(self.frames),
                           self.frame_flags, self.frame_stack, None if self.seeds is None else move(self.seeds))

    def to(self, device):
        return self._with(lambda t: t.to(device))

    def cpu(self):
        return self.to("cpu")

    def clone(self):
        return self._with(lambda t: t.clone())

    def state_dict(self):
        d = {"data": self.data, "count": self.count, "capacity": self.capacity}
        if self.frames is not None:
            d.update(frames=self.frames, frame_flags=self.frame_flags, frame_stack=self.frame_stack)
        if self.seeds is not None:
            d.update(seeds=self.seeds)
        return d

    @classmethod
    def from_state_dict(cls, d):
        return cls(d["data"], d["count"], d["capacity"], d.get("frames"), d.get("frame_flags", 0), d.get("frame_stack", 0), d.get("seeds"))

    def __len__(self):
        return self.count


class MiniWorldVecEnv:
    def __init__(self, env_id: str, num_envs: int, device_id: int = 0, domain_rand: bool = False,
                 want_depth: bool = False, seed: int = 0, autoreset: bool | str = True, obs_layout: str = "hwc",
                 rng: str = "auto", msaa: int = 8, final_obs: bool = False, frame_reuse: bool = True,
                 frame_cache: int = 4, frame_stack: int | None = None, stack_pad: str = "reset", **env_kwargs):
        """obs_layout: "hwc" uint8[N,H,W,3] (the env's observation), "cwh" uint8[N,3,W,H]
        (PyTorchObsWrapper, wrappers.py:24) or "grey" float64[N,H,W,1] (GreyscaleWrapper, wrappers.py:44):
        the raster kernel stores the frame in that layout, there is no extra pass.
        msaa: samples per pixel, 8 like the reference's FrameBuffer(80, 60, 8) (miniworld.py:515); 4 or 1 reproduce what the
        reference renders on a driver that clamps GL_MAX_SAMPLES (opengl.py:229-231) — same semantics, not the tuned path.
        rng: stream of the device-side resets. "pcg64" = numpy's own Generator(PCG64(SeedSequence(seed + i))) drawn in
        the reference's call order, so that env i IS the reference's env.reset(seed=seed + i) and its later episodes
        continue like env.reset(), per-step domain-randomisation draws included (every device generator);
        "philox" = the engine's counter-based stream; "auto" = pcg64 where implemented.
        autoreset: True or "same_step", "next_step", False (see the module's docstring); the mode is `autoreset_mode`
        ("same_step", "next_step" or "off").  "levels" (`autoreset_mode` "levels"): the engine itself resets nothing; after
        set_levels(bank) every step() restarts the envs whose episode it ended from record `next_level[i]` of the bank — two
        masked copy kernels behind the step, no draw and no host synchronisation.  What the caller sees is the same-step
        auto-reset: the observation (and `self.stack`) returned with terminated | truncated is the first one of the env's next
        level, reward and flags are the finished episode's last.
        "seeds" (`autoreset_mode` "seeds"): the engine's same-step auto-reset, seeded (mw_set_reset_seeds) — an env whose episode
        ends in a step starts the episode of the reference's env.reset(seed=next_seed[i]) in that step, generated on the device.
        `self.next_seed` and `self.episode_seed` are int64[N] device tensors (the engine reads the bits as uint64: keep them
        non-negative).  reset(seed=s) sets episode_seed[i] = s + i and next_seed[i] = s + N + i; behind every step, on the device
        and with no host value, episode_seed = where(done, next_seed, episode_seed) and next_seed += N where done — so left alone
        every env walks the seeds s + i, s + N + i, s + 2 N + i, ...  THE CALLER'S WRITES TO next_seed BETWEEN STEPS WIN: the engine
        reads next_seed[i] only when env i finishes, in that step (a level-replay sampler or a held-out evaluation writes its
        choices there).  Composes with final_obs, frame_stack, step(repeat=...) and rollout(); rollout(render=False) is refused.
        final_obs (same-step auto-reset only): every step also writes the terminal frame of each env whose episode ended in it
        into that env's row of `self.final_obs` (and its depth into `self.final_depth` with want_depth); the other rows keep
        what they held.  Costs a second, small frame of the finished envs in every step.
        frame_reuse: a step does not redraw an env whose frame did not change (a move into a wall, a pickup that finds nothing):
        its rows of `self.obs` / `self.depth` already hold that frame.  This env owns those tensors and passes them on every
        step, so it is on by default — TREAT THE RETURNED TENSORS AS READ-ONLY between steps (copy before normalising in
        place).  False, or MW_FRAME_REUSE=0 in the environment, draws every env on every step; `self.frame_reuse` tells which
        is in effect.  Results are bit for bit the same either way.
        frame_cache: the engine keeps every env's last `frame_cache` distinct drawn frames (0 .. 8) and copies one instead of
        drawing when the env is back in the state it shows — turn left then right, a move that a later one undoes; a third of the
        frames of a near-uniform policy.  Its own copies: nothing is asked of `self.obs`.  Costs num_envs x frame_cache x H x W x 3
        bytes of device memory (59 MB per slot at 4096 envs of 80x60; 78 MB more per slot with want_depth) and one more store of
        every drawn frame, which a policy that never returns to a state pays without gain.  0, or MW_FRAME_CACHE=0 in the
        environment, turns it off; `self.frame_cache` tells what is in effect.  Results are bit for bit the same either way.
        frame_stack=K (2 .. engine.MAX_STACK): the engine keeps every env's last K returned frames (Gymnasium's
        FrameStackObservation, SB3's VecFrameStack); `self.stack` is the ordered view [N, K, *obs.shape[1:]], oldest first, and with
        final_obs `self.final_stack` holds, for the envs whose episode ended in a step, the old stack with the terminal frame
        appended.  stack_pad: what a new episode's stack starts from, "reset" (K copies of its first frame) or "zero" (K - 1
        all-zero frames, then the frame).  One push per step() call, whatever `repeat` is; reset() rebuilds every stack."""
        import torch
        self.torch = torch
        self._check_arguments(env_id, autoreset, final_obs, obs_layout, rng, domain_rand, frame_stack, stack_pad)
        cls_name, self.generator, _, self.n_actions = _KIND[env_id]
        if cls_name == "Sign":
            domain_rand = False             # sign.py:92-98 fixes it
        self.env_id, self.num_envs = env_id, num_envs
        self.domain_rand, self.want_depth = domain_rand, want_depth
        self._make_template(cls_name, seed, env_kwargs)
        sc = scene_from_env(self.template)
        setup = build_config(env_id, self.template, sc, num_envs, device_id, domain_rand, msaa, self.autoreset_mode, rng)
        self.rng_mode = "pcg64" if setup.cfg.rng_mode == eng.RNG_PCG64 else "philox"
        self.engine = eng.Engine(setup.cfg)
        self._upload_assets(sc, setup)
        if self.generator == eng.GEN_PROGRAM:
            self._install_program(cls_name, sc)
        self._make_buffers(final_obs)
        self._set_frame_options(frame_reuse, frame_cache, final_obs)
        self._init_modes(cls_name, seed)

    host_autoreset = False      # every registered id is generated, ruled and auto-reset on the device

    def _check_arguments(self, env_id, autoreset, final_obs, obs_layout, rng, domain_rand, frame_stack, stack_pad):
        """The constructor's choices that need no world: refused before anything is made, kept as attributes otherwise."""
        if frame_stack is not None and (not isinstance(frame_stack, (int, np.integer)) or isinstance(frame_stack, bool)
                                        or not 2 <= frame_stack <= eng.MAX_STACK):
            raise ValueError(f"frame_stack must be an integer in 2 .. {eng.MAX_STACK} (or None), not {frame_stack!r}")
        if stack_pad not in ("reset", "zero"):
            raise ValueError(f"stack_pad must be 'reset' or 'zero', not {stack_pad!r}")
        self.frame_stack = None if frame_stack is None else int(frame_stack)
        self.stack_pad = stack_pad
        if not isinstance(autoreset, (bool, str)) or autoreset not in AUTORESET_MODES:
            raise ValueError(f"autoreset must be True, False, 'same_step', 'next_step', 'levels' or 'seeds', not {autoreset!r}")
        self.autoreset_mode = AUTORESET_MODES[autoreset]
        self.autoreset = self.autoreset_mode != "off"
        if final_obs and self.autoreset_mode not in ("same_step", "seeds"):
            why = {"next_step": "the terminal step returns the terminal frame itself",
                   "levels": "the terminal frame is in self.obs only between the engine's step and the level loads, and nothing copies the "
                             "finished envs' rows out yet",
                   "off": "nothing is auto-reset"}[self.autoreset_mode]
            raise ValueError(f"final_obs needs the same-step auto-reset (autoreset={autoreset!r}: {why})")
        if obs_layout not in ("hwc", "cwh", "grey"):
            raise ValueError(f"obs_layout must be 'hwc', 'cwh' or 'grey', not {obs_layout!r}")
        self.obs_layout = obs_layout
        if env_id not in _KIND:
            raise KeyError(f"{env_id!r} is not available in the batched engine yet; have {sorted(_KIND)}")
        if rng not in ("auto", "pcg64", "philox"):
            raise ValueError(f"rng={rng!r} is not available for {env_id} (domain_rand={domain_rand})")

    def _make_template(self, cls_name, seed, env_kwargs):
        """template world: geometry, textures, capacities (host-side world generation only)"""
        cls = getattr(_envs, cls_name)
        # (Sign fixes domain_rand=False itself and does not take the argument, sign.py:92-98)
        self._dr_kw = (lambda dr: {}) if cls_name == "Sign" else (lambda dr: {"domain_rand": dr})
        self.template = cls(host_only=True, **self._dr_kw(False), **env_kwargs)
        self.template.reset(seed=seed)
        self._cls, self._env_kwargs = cls, env_kwargs

    def _upload_assets(self, sc, setup):
        """the resident textures, the shared geometry set, the meshes the generator may draw"""
        from . import assets
        from .objmesh import ObjMesh
        self._tex_dr_variants = setup.textures if setup.tex_dr else None
        self.tex_ids, self.mesh_ids = {}, {}
        for i, variant in enumerate(setup.textures):
            self.tex_ids[variant] = i
            self.engine.upload_texture(i, assets.texture_rgb_bottom_up(variant))
        if setup.cfg.shared_geometry:
            self.engine.set_geometry(-1, polys_array(sc), sc["wall_segs"])
        for name in setup.meshes:
            self.mesh_ids[name] = len(self.mesh_ids)
            m = ObjMesh.get(name)
            self.engine.upload_mesh(self.mesh_ids[name], m.verts, m.norms, m.texcs, m.colors)

    def _install_program(self, cls_name, sc):
        """GEN_PROGRAM: the scene's own meshes, then the family's _gen_world as a placement program (genprog.py)"""
        from . import genprog
        mesh_map = upload_scene_meshes(self.engine, sc, self.mesh_ids, self.tex_ids)
        if cls_name == "RoomObjects":
            names = _ball_key_meshes()
            ops = genprog.room_objects_ops(0, 1, 2, self.mesh_ids[names[0]], self.mesh_ids[names[6]])
        else:
            ops = genprog.family_ops(self.template, _entity_slots(self.template).index, self.template.rooms.index)
        self.engine.set_gen_program(*genprog.compile_program(self.template, sc, self.tex_ids, mesh_map, ops))

    def _make_buffers(self, final_obs):
        """what a step writes: obs in the chosen layout, depth, reward, flags; with final_obs the terminal frames' own buffers"""
        torch, dev, n = self.torch, self.engine.device, self.num_envs
        H, W = self.template.obs_height, self.template.obs_width
        self.engine.set_obs_layout({"hwc": eng.OBS_HWC_U8, "cwh": eng.OBS_CWH_U8, "grey": eng.OBS_GREY_F64}[self.obs_layout])
        self.obs = self.engine.obs_buffer()
        self.depth = torch.zeros((n, H, W, 1), dtype=torch.float32, device=dev) if self.want_depth else None
        self.reward = torch.zeros(n, dtype=torch.float32, device=dev)
        self.terminated = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.truncated = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.substeps = None            # int32[N], made by the first step(actions, repeat > 1)
        self.step_rewards = self._step_rewards = None       # float32[T, N] of the last rollout(), a view of the buffer behind it
        self.trace = None               # name -> [T, N, ...] of the last rollout(trace=...), views of the buffers behind them
        self._trace_bufs = {}
        self.final_obs = self.final_depth = None
        if final_obs:
            self.final_obs = self.engine.obs_buffer()
            self.final_depth = torch.zeros_like(self.depth) if self.want_depth else None
            self.engine.set_final_obs(self.final_obs, self.final_depth)
        self._info_buf = self._final_info_buf = None
        self._state_bufs = {}           # state()'s tensors, one per field, made on first use
        self._nav_bufs = {}             # nav_query()'s tensors, made on first use
        self._lidar_bufs = {}           # lidar()'s offsets and result per (rays, fov), made on first use
        self._fork_buf = None           # fork()'s scratch records, made on first use
        self._fork_frames = None        # ... and its scratch frame records (fork(src, frames=True))
        self._done = self._done_b = self._done_i = None     # the finished envs of a step as uint8 / bool / int64 ("levels", "seeds")

    def _set_frame_options(self, frame_reuse, frame_cache, final_obs):
        """frame reuse, the frame cache and the frame stack, in that order"""
        torch, n = self.torch, self.num_envs
        self.frame_reuse = self.engine.set_frame_reuse(frame_reuse)
        if isinstance(frame_cache, bool) or not isinstance(frame_cache, (int, np.integer)) or not 0 <= frame_cache <= eng.MAX_FRAME_CACHE:
            raise ValueError(f"frame_cache must be an integer in 0 .. {eng.MAX_FRAME_CACHE}, not {frame_cache!r}")
        self.frame_cache = self.engine.set_frame_cache(frame_cache)
        self._ring = self.final_stack = None
        if self.frame_stack:
            K, frame = self.frame_stack, tuple(self.obs.shape[1:])
            self._ring = torch.zeros((n, 2 * K - 1) + frame, dtype=self.obs.dtype, device=self.engine.device)
            if final_obs:
                self.final_stack = torch.zeros((n, K) + frame, dtype=self.obs.dtype, device=self.engine.device)
            self.engine.set_frame_stack(K, {"reset": eng.STACK_PAD_RESET, "zero": eng.STACK_PAD_ZERO}[self.stack_pad], self._ring, self.final_stack)

    def _init_modes(self, cls_name, seed):
        """the seeds reset() hands out, the family's `info`, and what the "levels" and "seeds" auto-resets keep"""
        torch, n = self.torch, self.num_envs
        self._host_envs = None
        self._next_seed = seed
        # what the env's step() reports in `info` beside the observation (collecthealth.py:100, tmaze.py:89, ymaze.py:125)
        self._info_kind = _INFO_KIND.get(cls_name)
        self._info_slot = int(self.engine.cfg.goal_ent)
        # autoreset="levels": the bank (set_levels), the level each env plays and the one it gets when its episode ends
        self.levels = self.level = self.next_level = self.played_level = None
        self._level_gen = self._ones = None
        # autoreset="seeds": the seed each env gets when its episode ends (the engine reads it: mw_set_reset_seeds) and the one it plays
        self.next_seed = self.episode_seed = None
        if self.autoreset_mode == "seeds":
            self.next_seed = torch.arange(n, 2 * n, dtype=torch.int64, device=self.engine.device) + int(seed)
            self.episode_seed = torch.arange(n, dtype=torch.int64, device=self.engine.device) + int(seed)
            self._done_scratch()
            self._buffer("_done_i", (n,), torch.int64)
            self.engine.set_reset_seeds(self.next_seed)

    # ------------------------------------------------------------------ buffers and argument checks
    def _buffer(self, name, shape, dtype, store=None):
        """This env's own zeroed device tensor `name` — an attribute, or an entry of the dict `store` —, made on first use and made
        anew when `shape` asks for more rows than it has."""
        have = getattr(self, name) if store is None else store.get(name)
        if have is None or have.shape[0] < shape[0]:
            have = self.torch.zeros(shape, dtype=dtype, device=self.engine.device)
            if store is None:
                setattr(self, name, have)
            else:
                store[name] = have
        return have

    def _done_scratch(self):
        """the finished envs of a step as bytes and as booleans, behind a step of the "levels" and "seeds" modes"""
        self._buffer("_done", (self.num_envs,), self.torch.uint8)
        self._buffer("_done_b", (self.num_envs,), self.torch.bool)

    def _is_tensor(self, t, shape, dtype=None):
        """whether `t` is a contiguous tensor of `dtype` (default float64) and `shape` (None: any size there) on the engine's device"""
        torch = self.torch
        return (torch.is_tensor(t) and t.dtype == (dtype or torch.float64) and t.device == self.engine.device and t.is_contiguous()
                and len(t.shape) == len(shape) and all(s is None or s == d for s, d in zip(shape, t.shape)))

    def _copied_mask(self, mask):
        """reset_where / set_state_where: a host sequence or a uint8 / bool tensor anywhere, copied over as uint8[N] on the device"""
        torch = self.torch
        if not torch.is_tensor(mask):
            mask = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).astype(np.uint8))
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
        return mask.to(self.engine.device).contiguous()

    def _device_mask(self, mask, what):
        """nav_field / raycast: None, or a uint8 / bool [N] tensor already on the device; a bool is viewed as bytes (one byte per
        element, 0 / 1: no conversion kernel)"""
        torch = self.torch
        if mask is None:
            return None
        if (not torch.is_tensor(mask) or tuple(mask.shape) != (self.num_envs,) or mask.dtype not in (torch.uint8, torch.bool)
                or mask.device != self.engine.device):
            raise ValueError(f"{what}: mask is a uint8 or bool tensor [{self.num_envs}] on {self.engine.device}")
        return mask.view(torch.uint8) if mask.dtype == torch.bool else mask

    # ------------------------------------------------------------------ worlds from the host
    def host_generate(self, indices, seeds):
        """Host world generation (reference-compatible stream) for envs without a device generator."""
        if self._host_envs is None:
            self._host_envs = [None] * self.num_envs
        for i, s in zip(indices, seeds):
            env = self._host_envs[i]
            if env is None:
                env = self._cls(host_only=True, **self._dr_kw(self.domain_rand), **self._env_kwargs)
                self._host_envs[i] = env
            env.reset(seed=int(s))
            sc = scene_from_env(env)
            # with domain randomisation a world may draw a texture variant no earlier world used (concrete_2 ...):
            # upload it on first sight
            for v in [str(v) for v in sc["tex_names"]]:
                if v not in self.tex_ids:
                    from . import assets
                    self.tex_ids[v] = len(self.tex_ids)
                    self.engine.upload_texture(self.tex_ids[v], assets.texture_rgb_bottom_up(v))
            if not self.engine.cfg.shared_geometry:
                tex_map = {k: self.tex_ids[str(v)] for k, v in enumerate(sc["tex_names"])}
                self.engine.set_geometry(i, polys_array(sc, tex_map), sc["wall_segs"])
            mm = upload_scene_meshes(self.engine, sc, self.mesh_ids, self.tex_ids)
            self.engine.set_state(state_arrays([sc], self.engine.E, [mm]), first=i, count=1)
        if self.domain_rand:
            # the per-step forward_step / drift / turn_step draws (miniworld.py:677-680) come from the env's device
            # stream: seed it with the env's seed (not with the env index it got at creation)
            mask = np.zeros(self.num_envs, np.uint8)
            full = np.zeros(self.num_envs, np.uint64)
            for i, s_ in zip(indices, seeds):
                mask[i], full[i] = 1, int(s_)
            self.engine.reset(mask, full)

    # ------------------------------------------------------------------ API
    def reset(self, seed: int | None = None):
        """Reset every env (env i is seeded with seed + i); returns the observation tensor.
        autoreset="levels": every env starts level next_level[i] of the bank instead — the two masked loads with a mask of ones,
        nothing is generated or drawn, `seed` is not used — and next_level is refilled."""
        if self.autoreset_mode == "levels":
            self._need_levels("reset")
            self.terminated.zero_()
            self.truncated.zero_()
            self._start_levels(self._ones, frames=True)
            return self.obs
        if seed is not None:
            self._next_seed = seed
        if self.autoreset_mode == "seeds":
            # (the device reads these as uint64: a negative seed would become a huge one without a word)
            if self._next_seed < 0 or self._next_seed + 2 * self.num_envs > 2 ** 63:
                raise ValueError(f"reset: seed {self._next_seed} outside 0 .. 2^63 - 2 num_envs")
            self.torch.arange(self._next_seed, self._next_seed + self.num_envs, out=self.episode_seed)
            self.torch.arange(self._next_seed + self.num_envs, self._next_seed + 2 * self.num_envs, out=self.next_seed)
        seeds = np.arange(self.num_envs, dtype=np.uint64) + np.uint64(self._next_seed)
        self._next_seed += self.num_envs
        self.engine.reset(None, seeds)
        return self._redraw()

    def reset_where(self, mask, seeds):
        """The envs under `mask` (uint8[N] or bool[N]) start the episode of env.reset(seed=seeds[i]) (int64[N]), on the device and
        without a host synchronisation when both are device tensors (mw_reset_where); host sequences are copied over first, and a
        negative seed among them is refused.  seeds[i] is not read where mask[i] is 0.  Then the frame and the stack refresh of
        reset(); the other envs, their streams and their rows of `self.obs` stay as they are.  With autoreset="seeds",
        episode_seed follows; next_seed is the caller's.  Returns the observation tensor."""
        torch, dev = self.torch, self.engine.device
        if not torch.is_tensor(seeds):
            vals = [int(x) for x in np.asarray(seeds, dtype=object).ravel()]        # (Python integers: seeds up to 2^64 - 1 keep their bits)
            if any(not 0 <= x < 2 ** 64 for x in vals):
                raise ValueError("seeds: need non-negative integers below 2^64")
            seeds = torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64))
        elif seeds.device.type == "cpu" and seeds.dtype == torch.int64 and bool((seeds < 0).any()):
            raise ValueError("seeds: negative seed")
        mask, seeds = self._copied_mask(mask), seeds.to(device=dev, dtype=torch.int64).contiguous()
        self.engine.reset_where(mask, seeds)
        if self.episode_seed is not None:
            torch.where(mask != 0, seeds, self.episode_seed, out=self.episode_seed)
        return self._redraw()

    def _advance_seeds(self):
        """behind a step in seed mode, with no host value: episode_seed follows the envs that finished, their next_seed moves N on"""
        torch = self.torch
        torch.bitwise_or(self.terminated, self.truncated, out=self._done)
        torch.ne(self._done, 0, out=self._done_b)
        torch.where(self._done_b, self.next_seed, self.episode_seed, out=self.episode_seed)
        self._done_i.copy_(self._done_b)
        self.next_seed.add_(self._done_i, alpha=self.num_envs)

    @property
    def stack(self):
        """[N, K, *obs.shape[1:]], oldest frame first: a VIEW of the engine's ring (no copy, no kernel), computed per access from
        where the window lies — read-only and valid until the next step, like `self.obs`.  In the "cwh" layout
        `stack.reshape(N, 3 * K, W, H)` is a view too (the channel-stacked input of a CNN).  None without frame_stack."""
        if not self.frame_stack:
            return None
        first, _ = self.engine.stack_window()
        return self._ring[:, first:first + self.frame_stack]

    def step(self, actions, repeat: int = 1):
        """actions: integer torch tensor [N] (converted to contiguous int32 on the engine's device if needed).
        repeat > 1 (action repeat, up to engine.MAX_REPEAT): every env takes up to `repeat` steps with its action in one kernel
        launch and stops at the one that ends its episode; the observation is the frame after the last of them (after the
        auto-reset, as for a single step), the reward their sum, the flags the last one's, and `self.substeps` (int32[N] on
        the device) the number each env took — 0 for the reset step of autoreset="next_step".  max_episode_steps counts them.
        With frame_stack every call pushes its one frame; read `self.stack` afterwards."""
        levels = self.autoreset_mode == "levels"
        if levels:
            self._need_levels("step")
        if repeat == 1:
            self.engine.step(actions, self.obs, self.depth, self.reward, self.terminated, self.truncated)
        else:
            if self.substeps is None:
                self._buffer("substeps", (self.num_envs,), self.torch.int32)
            self.engine.step_repeat(actions, repeat, self.obs, self.depth, self.reward, self.terminated, self.truncated, self.substeps)
        if levels:
            self._finished_to_levels(frames=True)
        elif self.next_seed is not None:
            self._advance_seeds()
        return self.obs, self.reward, self.terminated, self.truncated

    TRACE_DEFAULT = ("agent_pos", "agent_dir", "carrying")

    def rollout(self, plans, render: bool = True, trace=None, trace_ent=None):
        """Open-loop rollout: plans is an integer torch tensor [T, N] (converted to contiguous int32 on the engine's device if
        needed), T in 1 .. engine.MAX_PLAN.  Env i takes plans[0, i], plans[1, i], ... in one kernel launch and stops at the step
        that ends its episode, exactly as T calls of step() would with a host that breaks on done (then the auto-reset, once).
        Returns (obs or None, reward, terminated, truncated): the reward is the sum, the flags the last executed step's;
        `self.substeps` (int32[N]) holds the executed counts and `self.step_rewards` (float32[T, N], a view of a buffer grown on
        demand) every step's own reward, 0 where the env did not execute it — what a planner discounts from.
        render=False is the frameless call, for planners that read no frames: nothing is drawn or pushed.  `self.obs`,
        `self.depth`, `self.stack` and the final buffers keep what they held and are STALE until the next drawn call (step(),
        rollout(render=True)), load_state(..., frames) or reset().
        autoreset="levels": the envs whose episode ended in the call restart from their next level behind it, as in step();
        render=False loads their states alone (the frames are stale by this call's contract; the state load marks the loaded
        envs' stacks, so their next push rebuilds them).
        trace: where the agent was after every step of the plan, for a planner's dense cost (the distance to a goal, a visitation
        count, a cell key) where the rewards are sparse.  True names ("agent_pos", "agent_dir", "carrying"); an iterable names any of
        those and "ent_pos", the position of ONE entity slot, `trace_ent` (default: the family's goal slot, engine.cfg.goal_ent —
        Hallway's box; a carried box moves with the agent).  `self.trace` is then a dict name -> device tensor, float64[T, N, 3] /
        float64[T, N] / int32[T, N] / float64[T, N, 3], views of buffers grown on demand: row k is the state behind the env's step k
        as state() would report it there — the terminal state on the step that ends an episode, in every auto-reset mode —, rows
        an env did not execute repeat its last one, and an env that executed nothing (next-step: it installed its world) repeats
        the state it entered with.  Written by the same one launch (mw_step_plan_trace); everything else the call returns is
        unchanged.  None: no trace, `self.trace` is None.  An unknown name, "ent_pos" on CollectHealth (its kits respawn behind
        the frame) or a slot outside 0 .. max_ents - 1 raises ValueError before any library call."""
        torch = self.torch
        names = None
        if trace is not None and trace is not False:
            names = self.TRACE_DEFAULT if trace is True else tuple(trace)
            if isinstance(trace, str) or not names:
                raise ValueError(f"trace: need True or an iterable of names out of {sorted(eng.TRACE_FIELDS)}, got {trace!r}")
            for name in names:
                if name not in eng.TRACE_FIELDS:
                    raise ValueError(f"trace: {name!r} is no trace field; have {sorted(eng.TRACE_FIELDS)}")
            slot = int(self.engine.cfg.goal_ent) if trace_ent is None else trace_ent
            if "ent_pos" in names:
                if self.engine.cfg.task == eng.TASK_COLLECT:
                    raise ValueError("trace: 'ent_pos' on CollectHealth (a consumed kit respawns behind the frame, not inside the step)")
                if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= slot < self.engine.cfg.max_ents:
                    raise ValueError(f"trace_ent: need an entity slot in 0 .. {self.engine.cfg.max_ents - 1}, got {trace_ent!r}")
        if plans.dim() != 2 or plans.shape[1] != self.num_envs:
            raise ValueError(f"plans: need an integer tensor [T, {self.num_envs}], got {tuple(plans.shape)}")
        T = int(plans.shape[0])
        if not 1 <= T <= eng.MAX_PLAN:
            raise ValueError(f"plans: T = {T} outside 1 .. {eng.MAX_PLAN}")
        if self.substeps is None:
            self._buffer("substeps", (self.num_envs,), torch.int32)
        if self._step_rewards is None or self._step_rewards.shape[0] < T:     # (_buffer's own rule, asked here first: every rollout's path)
            self._buffer("_step_rewards", (T, self.num_envs), torch.float32)
        self.step_rewards = self._step_rewards[:T]
        obs, depth = (self.obs, self.depth) if render else (None, None)
        if self.next_seed is not None and not render:
            raise ValueError("rollout(render=False) with autoreset='seeds': a frameless call cannot seed the envs that finish in it")
        if self.autoreset_mode == "levels":
            self._need_levels("rollout")
        if names is None:
            self.trace = None
            self.engine.step_plan(plans, obs, depth, self.reward, self._step_rewards, self.terminated, self.truncated, self.substeps)
        else:
            bufs = {name: self._buffer(name, (T, self.num_envs) + eng.TRACE_FIELDS[name][1], eng.torch_dtype(eng.TRACE_FIELDS[name][0]), self._trace_bufs)
                    for name in names}
            self.trace = {name: b[:T] for name, b in bufs.items()}
            self.engine.step_plan_trace(plans, obs, depth, self.reward, self._step_rewards, self.terminated, self.truncated, self.substeps,
                                        trace=bufs, ent_slot=int(slot) if "ent_pos" in names else 0)
        if self.autoreset_mode == "levels":
            self._finished_to_levels(frames=render)
        elif self.next_seed is not None:
            self._advance_seeds()
        return obs, self.reward, self.terminated, self.truncated

    # ------------------------------------------------------------------ level sets
    def make_levels(self, seeds):
        """A bank of levels: record l of the returned EnvSnapshot IS the reference's env.reset(seed=seeds[l]) on the PCG64 stream —
        world, agent, random stream, pre-generated next world — together with its first observation (depth, frame stack) as frame
        records under this env's frame flags.  `seeds` is an integer sequence or tensor of any length L, more than num_envs too: the
        bank is built num_envs levels at a time (engine.reset with the seeds, a render, a stack refresh, then mw_snapshot_save_at /
        mw_snapshot_save_frames_at into records base .. base + m - 1).  `snap.seeds` keeps the seeds (int64).
        Afterwards this env's own state is the last chunk's: call reset() or set_levels() next.
        A record carries the env's random stream, so under domain randomisation every replay of a level draws the same per-step
        noise; a bank that keeps the level but not the stream is not built here."""
        torch = self.torch
        if isinstance(seeds, torch.Tensor):
            seeds_np = seeds.detach().cpu().numpy()
        else:
            seeds_np = np.asarray(seeds)
        if seeds_np.ndim != 1 or seeds_np.size == 0 or seeds_np.dtype.kind not in "iu":
            raise ValueError(f"seeds: need a non-empty 1-D integer sequence, got {seeds_np.dtype} {seeds_np.shape}")
        if seeds_np.dtype.kind == "i" and (seeds_np < 0).any():
            raise ValueError("seeds: negative seed")
        seeds_np = seeds_np.astype(np.uint64)
        L, N, dev = int(seeds_np.size), self.num_envs, self.engine.device
        flags = self._frame_flags()
        data = torch.zeros(self.engine.snapshot_bytes(L), dtype=torch.uint8, device=dev)
        fdata = torch.zeros(self.engine.snapshot_frames_bytes(L, flags), dtype=torch.uint8, device=dev)
        for base in range(0, L, N):
            m = min(N, L - base)
            mask, full = np.zeros(N, np.uint8), np.zeros(N, np.uint64)
            mask[:m], full[:m] = 1, seeds_np[base:base + m]
            self.engine.reset(mask, full)
            self._redraw()
            recs = torch.arange(base, base + m, dtype=torch.int32, device=dev)     # (envs None: env k is item k, k < m)
            self.engine.snapshot_save_at(data, L, None, recs)
            self.engine.snapshot_save_frames_at(fdata, L, self.obs, self.depth, flags, None, recs)
        return EnvSnapshot(data, L, L, fdata, flags, self.frame_stack or 0, torch.from_numpy(seeds_np.astype(np.int64)).to(dev))

    def _check_frame_config(self, snap, what):
        if snap.frames is None:
            raise ValueError(f"{what}: the snapshot holds no frame records (make_levels, save_state(frames=True))")
        if snap.frame_flags != self._frame_flags() or snap.frame_stack != (self.frame_stack or 0):
            raise ValueError(f"{what}: the snapshot's frame records (flags {snap.frame_flags}, frame_stack {snap.frame_stack}) are not this "
                             f"env's (flags {self._frame_flags()}, frame_stack {self.frame_stack or 0}: want_depth / frame_stack differ)")

    def set_levels(self, snap, generator=None):
        """autoreset="levels": `snap` (make_levels, or any snapshot with frame records of this env's frame configuration) becomes the
        bank finished envs restart from; its buffers are moved to the device once.  Creates `self.level` and `self.next_level`, int32[N]
        on the device: level[i] is the record env i is playing (`self.played_level`: the one it played in the step that just ended,
        which differs for the envs that step finished), next_level[i] the one it gets when its episode ends — drawn uniformly
        from 0 .. len(snap) - 1 with torch.randint(generator=generator) behind every step, and the caller's to overwrite between
        steps (a level-replay sampler writes its choice there, on the device).  Call reset() next."""
        torch = self.torch
        if self.autoreset_mode != "levels":
            raise RuntimeError(f"set_levels needs autoreset='levels' (this env: {self.autoreset_mode!r})")
        self._check_frame_config(snap, "set_levels")
        if snap.count < 1:
            raise ValueError("set_levels: the snapshot holds no records")
        dev, N = self.engine.device, self.num_envs
        self.levels = snap if snap.data.device == dev and snap.frames.device == dev else snap.to(dev)
        self._level_gen = generator
        self.level, self.next_level, self.played_level = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(3))
        self._done_scratch()
        self._ones = torch.ones(N, dtype=torch.uint8, device=dev)
        self._draw_next_levels()

    def _need_levels(self, what):
        if self.levels is None:
            raise RuntimeError(f"{what}() with autoreset='levels' before set_levels(): there is no bank to restart finished envs from")

    def _draw_next_levels(self):
        self.torch.randint(0, self.levels.count, (self.num_envs,), generator=self._level_gen, out=self.next_level)

    def _start_levels(self, mask, frames):
        """the envs under `mask` (uint8[N], device) start level next_level[i]: states, then frames; then the bookkeeping"""
        torch, bank = self.torch, self.levels
        self.engine.snapshot_load_where(bank.data, bank.count, bank.capacity, mask, self.next_level)
        if frames:
            self.engine.snapshot_load_frames_where(bank.frames, bank.count, bank.capacity, mask, self.next_level, self.obs, self.depth, bank.frame_flags)
        torch.ne(mask, 0, out=self._done_b)
        self.played_level.copy_(self.level)
        torch.where(self._done_b, self.next_level, self.level, out=self.level)
        self._draw_next_levels()

    def _finished_to_levels(self, frames):
        """behind a step in level mode, with no host synchronisation: done, the terminal infos, the two loads, level, next_level"""
        torch = self.torch
        torch.bitwise_or(self.terminated, self.truncated, out=self._done)
        if self._info_kind is not None:
            # the finished episodes' own values, before the loads replace the states they are read from (final_infos)
            now = self.infos()[self._info_kind]
            kept = self._info_buffer("_final_info_buf")
            done = self._done.bool()
            torch.where(done if now.dim() == 1 else done[:, None], now, kept, out=kept)
        self._start_levels(self._done, frames)

    def _info_buffer(self, name):
        """what get_info / get_final_info fill for this env's `info` key, made on first use: health int32[N], goal_pos float64[N, 3]"""
        if self._info_kind == "health":
            return self._buffer(name, (self.num_envs,), self.torch.int32)
        return self._buffer(name, (self.num_envs, 3), self.torch.float64)

    # ------------------------------------------------------------------ save / restore / fork
    def save_state(self, envs=None, capacity: int | None = None, frames: bool = False, into=None, records=None):
        """The complete state of the envs `envs` (an integer sequence or tensor; None: all of them, in order) as an EnvSnapshot on
        the device: everything that decides their future — poses, entities, step counts, the random stream, pending removals and
        resets, the Maze's own geometry, the pre-generated next world — but no frames (include/mwengine.h: mw_snapshot_save).  One
        kernel on the current stream; nothing in this env changes.
        capacity: the records the buffer is laid out for (default: the number saved).  One load_state call moves at most that many
        envs, so a snapshot of ONE state that is to be loaded into many envs at once ("reset all of them to this cell") is taken
        with capacity=num_envs: `vec.load_state(vec.save_state([i], capacity=n), records=torch.zeros(n, dtype=torch.int32))`.
        frames=True: a second kernel also saves what the agent saw — the envs' rows of `self.obs`, of `self.depth` with want_depth,
        and their frame stacks with frame_stack (mw_snapshot_save_frames) — into `snap.frames`; load_state() then puts those
        frames back instead of drawing new ones.
        into=snap, records=idx: the envs are saved into the records idx[k] (distinct) of an EXISTING snapshot on this env's device
        instead (mw_snapshot_save_at), their frames too when `snap` has frame records — they must be of this env's frame
        configuration —, and `snap` is returned; its other records keep what they held and its count grows to cover the highest
        record named.  A running loop adds states to a bank this way: an archive of cells, a curriculum of reached states.
        ValueError for a snapshot of another frame configuration, for indices of the wrong length, and for `into` with `capacity`."""
        torch = self.torch
        if into is not None:
            return self._save_into(into, envs, records, capacity)
        if records is not None:
            raise ValueError("save_state: records needs into=<snapshot>")
        envs, count = self._named_envs(envs)
        capacity = count if capacity is None else int(capacity)
        if capacity < count:
            raise ValueError(f"capacity {capacity} < the {count} records to save")
        data = torch.zeros(self.engine.snapshot_bytes(capacity), dtype=torch.uint8, device=self.engine.device)
        self.engine.snapshot_save(data, capacity, envs)
        if not frames:
            return EnvSnapshot(data, count, capacity)
        flags = self._frame_flags()
        fdata = torch.zeros(self.engine.snapshot_frames_bytes(capacity, flags), dtype=torch.uint8, device=self.engine.device)
        self.engine.snapshot_save_frames(fdata, capacity, self.obs, self.depth, flags, envs)
        return EnvSnapshot(data, count, capacity, fdata, flags, self.frame_stack or 0)

    def _named_envs(self, envs):
        """(the envs a save names, as a tensor or None for all of them in order; how many they are)"""
        envs = None if envs is None else self.torch.as_tensor(envs)
        return envs, self.num_envs if envs is None else int(envs.numel())

    def _save_into(self, snap, envs, records, capacity):
        torch = self.torch
        if capacity is not None:
            raise ValueError("save_state: into=<snapshot> has its own capacity; capacity cannot be given with it")
        if records is None:
            raise ValueError("save_state: into=<snapshot> needs records=<the record indices>")
        if snap.frames is not None:
            self._check_frame_config(snap, "save_state(into=...)")
        envs, count = self._named_envs(envs)
        rec_host = torch.as_tensor(records)
        if rec_host.dim() != 1 or int(rec_host.numel()) != count:
            raise ValueError(f"save_state: {tuple(rec_host.shape)} record indices for {count} envs")
        if count > snap.capacity:
            raise ValueError(f"save_state: {count} records into a snapshot of capacity {snap.capacity}")
        if snap.data.device != self.engine.device or (snap.frames is not None and snap.frames.device != self.engine.device):
            raise ValueError(f"save_state: into=<snapshot> must live on {self.engine.device} (snap.to(device))")
        envs, recs = self.engine._index_tensor(envs, "envs"), self.engine._index_tensor(records, "records")
        self.engine.snapshot_save_at(snap.data, snap.capacity, envs, recs)
        if snap.frames is not None:
            self.engine.snapshot_save_frames_at(snap.frames, snap.capacity, self.obs, self.depth, snap.frame_flags, envs, recs)
        if rec_host.device.type == "cpu" and count:     # (device indices: the caller keeps count; nothing is read back here)
            snap.count = max(snap.count, min(int(rec_host.max()) + 1, snap.capacity))
        return snap

    def _frame_flags(self):
        """the engine.SNAPF_* bits of this env's frame records: depth with want_depth, the stacks with frame_stack"""
        return (eng.SNAPF_DEPTH if self.depth is not None else 0) | (eng.SNAPF_STACK if self.frame_stack else 0)

    def load_state(self, snap, envs=None, records=None, frames: bool | None = None):
        """Env envs[k] becomes record records[k] of `snap` (envs=None: env k; records=None: record k; the envs must be distinct,
        records may repeat; one call moves at most `snap.capacity` envs) and continues bit for bit as the env the record was taken from would have — on this env or on another
        one of the same configuration, whatever its num_envs.  Draws the new frames (and rebuilds the loaded envs' frame stacks as
        reset() does) and returns `self.obs`; rewards and flags are left alone.
        frames: None uses the snapshot's frame records if it has any (save_state(frames=True)), False never does, True insists
        (ValueError without them).  With them nothing is drawn and no stack is rebuilt: the loaded envs' rows of `self.obs` /
        `self.depth` and their stacks are copied back (mw_snapshot_load, mw_snapshot_load_frames).  What differs from the redraw:
        the observation is the one the record's source RETURNED — a picked-up object's last appearance included, which a frame of
        the restored state does not show — and `self.stack` is the source's stack, not a new episode's.  The snapshot's frame flags
        and stack depth must be this env's (want_depth, frame_stack): ValueError otherwise, before anything is launched."""
        if frames is None:
            frames = snap.frames is not None
        if frames:
            self._check_frame_config(snap, "load_state")
        dev = self.engine.device
        data = snap.data if snap.data.device == dev else snap.data.to(dev)
        if frames:      # (both loads take the same indices: made device tensors once)
            fdata = snap.frames if snap.frames.device == dev else snap.frames.to(dev)
            envs, records = self.engine._index_tensor(envs, "envs"), self.engine._index_tensor(records, "records")
        self.engine.snapshot_load(data, snap.count, snap.capacity, envs, records)
        if not frames:
            return self._redraw()
        self.engine.snapshot_load_frames(fdata, snap.count, snap.capacity, self.obs, self.depth, snap.frame_flags, envs, records)
        return self.obs

    def fork(self, src, frames: bool = False):
        """src: integer tensor [N].  Env j becomes a copy of env src[j] (its stream included: copies given the same actions stay
        identical) — a whole-batch save into scratch records of this env's own and a load through `src`, two kernels and a frame;
        returns `self.obs`.
        frames=True: no frame is drawn.  Env j's frame after the fork IS env src[j]'s, and it is already on the device: the frames
        are saved and loaded through `src` like the states — save, save_frames, load, load_frames, four copy kernels.  What differs
        from the redraw: env j's observation (and depth) is the one env src[j]'s last step returned — a picked-up object's last
        appearance included — and its frame stack is env src[j]'s, so a policy that reads `self.stack` sees in the copy what it saw
        in the source."""
        eng_ = self.engine
        n = self.num_envs
        if self._fork_buf is None:
            self._fork_buf = self.torch.empty(eng_.snapshot_bytes(n), dtype=self.torch.uint8, device=eng_.device)
        src = eng_._index_tensor(src, "src", n)
        flags = self._frame_flags()
        if frames and self._fork_frames is None:
            self._fork_frames = self.torch.empty(eng_.snapshot_frames_bytes(n, flags), dtype=self.torch.uint8, device=eng_.device)
        eng_.snapshot_save(self._fork_buf, n)
        if frames:
            eng_.snapshot_save_frames(self._fork_frames, n, self.obs, self.depth, flags)
        eng_.snapshot_load(self._fork_buf, n, n, None, src)
        if not frames:
            return self._redraw()
        eng_.snapshot_load_frames(self._fork_frames, n, n, self.obs, self.depth, flags, None, src)
        return self.obs

    # ------------------------------------------------------------------ state views
    STATE_DEFAULT = ("agent_pos", "agent_dir", "carrying", "step_count", "ent_kind", "ent_pos", "ent_dir")

    def state(self, fields=None):
        """The envs' own state as device tensors — what code around the reference reads as env.agent.pos / .dir / .carrying,
        env.entities[k].pos, env.step_count: {"agent_pos": float64[N, 3], "agent_dir": float64[N], "carrying": int32[N] (entity slot
        or -1), "step_count": int32[N], "ent_kind": int32[N, E] (engine.ENT_*, ENT_NONE = empty or removed), "ent_pos":
        float64[N, E, 3], "ent_dir": float64[N, E]} by default; `fields` is any subset of the names of engine.get_state() ("cam",
        "light", "num_picked_up", "ent_mesh", "ent_static", "ent_geom", "extent" beside those).  One gather kernel on the engine's
        stream (mw_get_state_device), no synchronisation and no host value: an expert, a visitation count or an archive's cell key
        is computed from it in torch behind the step.  The tensors are this env's own, reused between calls: valid until the next
        state() call that names the field.  The values are those of the state the device holds (as for infos(): with the same-step
        auto-reset an env that just finished reports its new episode; with the next-step auto-reset it reports the finished one
        until its next step installs the new episode)."""
        e = self.engine
        names = self.STATE_DEFAULT if fields is None else tuple(fields)
        out = {}
        for name in names:
            if name not in eng.STATE_FIELDS:
                raise ValueError(f"state: {name!r} is no state field; have {sorted(eng.STATE_FIELDS)}")
            dt, shp = eng.STATE_FIELDS[name]
            out[name] = self._buffer(name, (self.num_envs,) + shp(e.E), eng.torch_dtype(dt), self._state_bufs)
        if not out:
            raise ValueError("state: no field named")
        return e.get_state_device(out)

    def set_state_where(self, mask, **fields):
        """The envs under `mask` (uint8[N] or bool[N]) get row i of every field given — agent_pos=float64[N, 3], agent_dir=float64[N],
        ent_pos=float64[N, E, 3], carrying=int32[N], ...: the names, shapes and dtypes of state() — written into their state, on the
        device and without a host synchronisation when everything is a device tensor (mw_set_state_where); host sequences and bool
        masks are copied over first.  Mid-episode injection, as engine.set_state(): teleporting the agents of chosen envs, a
        start-state curriculum, goal relabelling; no consistency is made between fields, and rows where mask[i] is 0 are not read.
        A device tensor of the wrong dtype or shape is refused, never converted.  Then the frame and the stack refresh of reset();
        the other envs, their cached frames and their rows of `self.obs` stay as they are.  In the "seeds" and "levels" modes
        episode_seed and level are left alone: the env is still playing that episode.  Returns the observation tensor."""
        torch, dev = self.torch, self.engine.device
        if not fields:
            raise ValueError("set_state_where: no field given")
        arrays = {}
        for name, val in fields.items():
            if name not in eng.STATE_FIELDS:
                raise ValueError(f"set_state_where: {name!r} is no state field; have {sorted(eng.STATE_FIELDS)}")
            dt, shp = eng.STATE_FIELDS[name]
            if not torch.is_tensor(val):
                val = torch.from_numpy(np.ascontiguousarray(np.asarray(val, dtype=dt))).to(dev)
            arrays[name] = val
        mask = self._copied_mask(mask)
        # (the tensors are checked before the first library call: a wrong one leaves the engine as it was)
        for name, t in arrays.items():
            self.engine._state_tensor(t, name, self.num_envs)
        self.engine.set_state_where(mask, arrays)
        return self._redraw()

    # ------------------------------------------------------------------ navigation fields
    NAV_OBSTACLES = {"walls": 0, "walls+entities": eng.NAV_ENTITIES}

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
            if target is not None or margin is not None or reach is not None or (cell, obstacles) != (0.25, "walls"):
                raise ValueError("nav_field: with `into` the field's own target and parameters are used: pass only mask")
            field, params, target = into.field, into.params, into.target
        else:
            if obstacles not in self.NAV_OBSTACLES:
                raise ValueError(f"nav_field: obstacles {obstacles!r}; have {sorted(self.NAV_OBSTACLES)}")
            if not (isinstance(cell, (int, float)) and cell > 0 and math.isfinite(cell)):
                raise ValueError(f"nav_field: cell {cell!r} must be a positive length")
            margin = cell / 2 if margin is None else margin
            if not (margin >= 0 and math.isfinite(margin)):
                raise ValueError(f"nav_field: margin {margin!r} < 0")
            if target is None:
                target = int(e.cfg.goal_ent)
                if target < 0:
                    raise ValueError("nav_field: this env has no goal entity: name a target slot or points")
            if torch.is_tensor(target):
                if not self._is_tensor(target, (self.num_envs, 3)):
                    raise ValueError(f"nav_field: point targets are a contiguous float64 tensor [{self.num_envs}, 3] on {e.device}")
                if reach is None or not (reach > 0 and math.isfinite(reach)):
                    raise ValueError(f"nav_field: point targets need reach > 0, got {reach!r}")
            elif isinstance(target, (int, np.integer)) and not isinstance(target, bool):
                target = int(target)
                if not 0 <= target < e.cfg.max_ents:
                    raise ValueError(f"nav_field: target slot {target} outside 0 .. {e.cfg.max_ents - 1}")
                if reach is not None:
                    raise ValueError("nav_field: a slot target's reach is the env's own near() distance: pass no reach")
            else:
                raise ValueError(f"nav_field: target is None, an entity slot or a float64[N, 3] device tensor, not {type(target).__name__}")
            t = self.template
            gx = max(1, math.ceil((float(t.max_x) - float(t.min_x)) / cell))
            gz = max(1, math.ceil((float(t.max_z) - float(t.min_z)) / cell))
            if gx * gz > eng.NAV_MAX_CELLS:
                raise ValueError(f"nav_field: {gx} x {gz} cells > {eng.NAV_MAX_CELLS}: use a larger cell")
            params = eng.MwNavParams(float(cell), float(margin), float(reach or 0.0), gx, gz, self.NAV_OBSTACLES[obstacles],
                                     target if isinstance(target, int) else 0)
            # (0xFFFF throughout; filled as int16: the 16-bit unsigned type has few kernels of its own)
            field = torch.full((self.num_envs, gz, gx), -1, dtype=torch.int16, device=e.device).view(torch.uint16)
        mask = self._device_mask(mask, "nav_field")
        out = into if into is not None else NavField(field, params, target, obstacles)
        e.nav_build(params, field, mask, out.points)
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
    SEEN_OBSTACLES = {"walls": 0, "walls+entities": eng.SEEN_ENTITIES}

    def default_fov(self):
        """The horizontal field of view of the default camera in radians: 2 atan(tan(fov_y / 2) * width / height) from the vertical
        field of view the env's parameters default to (cam_fov_y, 60 degrees) and the observation's aspect."""
        cfg = self.engine.cfg
        return 2.0 * math.atan(math.tan(math.radians(float(cfg.cam_fov_y.default)) / 2.0) * float(cfg.obs_width) / float(cfg.obs_height))

    def seen_map(self, cell=0.25, max_range=10.0, fov=None, obstacles="walls", like=None):
        """An empty explored-area map over each env's floor plan: a SeenMap, which seen_update() fills.

        cell       metres per cell; gx, gz follow from the template world's extent exactly as in nav_field()
        like       a NavField whose grid (cell, gx, gz) the map adopts, so that map and field line up cell for cell; pass no cell then
        max_range  how far the agent sees, in metres
        fov        the horizontal opening angle of sight in radians, 0 < fov <= 2 pi, about the agent's heading; None: default_fov(),
                   the horizontal field of view of the default camera — the vertical field of view the parameters default to and
                   the observation's aspect, so that a cell is seen when the frame could show its floor point.  2 pi: all round.
        obstacles  "walls", or "walls+entities": every listed entity but the carried one blocks the line of sight too, as a disc of
                   full height
        A cell counts as seen once its centre is within max_range and the cone and the straight line from the agent to it meets no
        obstacle (include/mwengine.h, "explored-area maps").  ValueError for arguments that make no map; nothing is launched."""
        torch, e = self.torch, self.engine
        if obstacles not in self.SEEN_OBSTACLES:
            raise ValueError(f"seen_map: obstacles {obstacles!r}; have {sorted(self.SEEN_OBSTACLES)}")
        if not (isinstance(max_range, (int, float)) and not isinstance(max_range, bool) and max_range > 0 and math.isfinite(max_range)):
            raise ValueError(f"seen_map: max_range {max_range!r} must be a positive finite length")
        fov = self.default_fov() if fov is None else fov
        if not (isinstance(fov, (int, float)) and not isinstance(fov, bool) and 0 < fov <= 2 * math.pi):
            raise ValueError(f"seen_map: fov {fov!r} outside 0 .. 2 pi radians")
        cos_half = -1.0 if fov == 2 * math.pi else math.cos(fov / 2)
        if like is not None:
            if not isinstance(like, NavField):
                raise ValueError("seen_map: `like` must be a NavField")
            if cell != 0.25:
                raise ValueError("seen_map: with `like` the field's own grid is used: pass no cell")
            cell, gx, gz = like.cell, like.gx, like.gz
        else:
            if not (isinstance(cell, (int, float)) and not isinstance(cell, bool) and cell > 0 and math.isfinite(cell)):
                raise ValueError(f"seen_map: cell {cell!r} must be a positive length")
            t = self.template
            gx = max(1, math.ceil((float(t.max_x) - float(t.min_x)) / cell))
            gz = max(1, math.ceil((float(t.max_z) - float(t.min_z)) / cell))
            if gx * gz > eng.NAV_MAX_CELLS:
                raise ValueError(f"seen_map: {gx} x {gz} cells > {eng.NAV_MAX_CELLS}: use a larger cell")
        params = eng.MwNavParams(float(cell), 0.0, 0.0, int(gx), int(gz), 0, 0)
        n = self.num_envs
        return SeenMap(torch.zeros((n, int(gz), int(gx)), dtype=torch.uint8, device=e.device), torch.zeros(n, dtype=torch.int32, device=e.device),
                       torch.zeros(n, dtype=torch.int32, device=e.device), params, float(max_range), float(cos_half), obstacles)

    def _seen_flags(self, t, what):
        """seen_update's clear and mask: None, or a uint8 / bool [N] tensor on the device; a bool is copied over as bytes"""
        torch = self.torch
        if t is None:
            return None
        if (not torch.is_tensor(t) or tuple(t.shape) != (self.num_envs,) or t.dtype not in (torch.uint8, torch.bool) or t.device != self.engine.device):
            raise ValueError(f"seen_update: {what} is a uint8 or bool tensor [{self.num_envs}] on {self.engine.device}")
        return self._copied_mask(t) if t.dtype == torch.bool else t

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
        clear, mask = self._seen_flags(clear, "clear"), self._seen_flags(mask, "mask")
        self.engine.seen_update(seen.params, seen.max_range, seen.cos_half, self.SEEN_OBSTACLES[seen.obstacles], seen.seen, seen.count, seen.new, mask, clear)
        return seen.new

    # ------------------------------------------------------------------ ray casts
    RAY_OBSTACLES = {"walls": 0, "walls+entities": eng.RAY_ENTITIES}

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
        if not (isinstance(max_t, (int, float)) and not isinstance(max_t, bool) and max_t > 0 and math.isfinite(max_t)):
            raise ValueError(f"raycast: max_t {max_t!r} must be a positive finite number")
        if not (isinstance(radius, (int, float)) and not isinstance(radius, bool) and radius >= 0 and math.isfinite(radius)):
            raise ValueError(f"raycast: radius {radius!r} must be a finite number >= 0")
        if obstacles not in self.RAY_OBSTACLES:
            raise ValueError(f"raycast: obstacles {obstacles!r}; have {sorted(self.RAY_OBSTACLES)}")
        mask = self._device_mask(mask, "raycast")
        # the result's tensors: name -> (dtype, shape, what an unmasked row holds)
        want = {"t": (torch.float64, (n, rays), float(max_t)), "hit": (torch.int32, (n, rays), -1)}
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
        params = eng.MwRayParams(float(max_t), float(radius), rays, self.RAY_OBSTACLES[obstacles])
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
        if not (isinstance(rays, (int, np.integer)) and not isinstance(rays, bool) and 1 <= rays <= eng.RAY_MAX):
            raise ValueError(f"lidar: rays {rays!r} outside 1 .. {eng.RAY_MAX}")
        if not (isinstance(fov, (int, float)) and not isinstance(fov, bool) and 0 < fov <= 2 * math.pi):
            raise ValueError(f"lidar: fov {fov!r} outside 0 .. 2 pi radians")
        rays = int(rays)
        key = (rays, float(fov))
        if key not in self._lidar_bufs:
            if fov < 2 * math.pi:
                off = [0.0] if rays == 1 else [-fov / 2 + k * fov / (rays - 1) for k in range(rays)]
            else:
                off = [k * 2 * math.pi / rays for k in range(rays)]
            self._lidar_bufs[key] = [torch.tensor(off, dtype=torch.float64, device=e.device), None]
        buf = self._lidar_bufs[key]
        buf[1] = self.raycast(offsets=buf[0], max_t=max_range, radius=radius, obstacles=obstacles, into=buf[1])
        return buf[1]

    def _redraw(self):
        self.engine.render(self.obs, self.depth)
        if self.frame_stack:
            self.engine.stack_refresh(self.obs)
        return self.obs

    def infos(self):
        """The batched `info` of the last step as device tensors: {"health": int32[N]} for CollectHealth (collecthealth.py:100),
        {"goal_pos": float64[N, 3]} for TMaze / YMaze (the box's position, tmaze.py:89, ymaze.py:125), {} for the other envs
        (miniworld.py:730 returns an empty dict).  One small gather kernel on the engine's stream; the values are those of the
        state the device holds (with the same-step auto-reset an env that just finished reports its new episode — the finished
        episode's own values: final_infos —; with the next-step auto-reset it reports the finished one)."""
        return self._fill_info("_info_buf", self.engine.get_info, self._info_slot)

    def final_infos(self):
        """The `info` each env's last FINISHED episode ended with ({"health": …} / {"goal_pos": …} / {}), as the step kernel kept it
        before the same-step auto-reset installed the next world (mw_get_final_info); rows of envs that have not finished an episode yet
        are undefined (mask them with terminated | truncated of the step)."""
        if self._info_kind is not None and self.autoreset_mode == "levels":
            # (kept by step() itself before the level loads; the engine installs nothing here)
            return {self._info_kind: self._info_buffer("_final_info_buf")}
        return self._fill_info("_final_info_buf", self.engine.get_final_info)

    def _fill_info(self, name, get, *slot):
        """infos() and final_infos(): the family's buffer `name` filled by the engine's getter — get(health, position, *slot)"""
        if self._info_kind is None:
            return {}
        buf = self._info_buffer(name)
        if self._info_kind == "health":
            get(buf)
        else:
            get(None, buf, *slot)
        return {self._info_kind: buf}

    def reset_pending(self):
        """uint8[N] device tensor: 1 = the env's last step ended its episode and its next step (autoreset="next_step") installs
        the next world instead of stepping — its action is ignored and its transition is no transition of the env (mask it out
        of a replay buffer).  All zeros in the other modes."""
        return self.engine.get_reset_pending()

    def frame_source(self):
        """uint8[N] on the device: where each env's frame of the last step came from — 0 drawn, 1 left alone as clean, 2 + j copied
        from slot j of the frame cache."""
        return self.engine.get_frame_source()

    def frame_clean(self):
        """uint8[N] device tensor: 1 = the env's observation of the last step is bit for bit the one before it (its state did not
        change), so per-frame work of the consumer's own can be skipped for it too."""
        return self.engine.get_frame_clean()

    def render_top_view(self, render_agent=True):
        """uint8[N,H,W,3] map views (render_top_view, miniworld.py:1088-1175) of every env."""
        layout = self.engine.obs_layout
        self.engine.set_obs_layout(eng.OBS_HWC_U8)
        out = self.engine.obs_buffer()
        self.engine.render_top(out, None, render_agent)
        self.engine.set_obs_layout(layout)
        return out

    def get_visible_ents(self):
        """bool[N, max_ents]: which entity slots each agent currently sees (get_visible_ents,
        miniworld.py:1238-1333: occlusion queries around 0.2 m proxy boxes)."""
        return self.engine.visible_ents().bool()

    def close(self):
        self.engine.close()
