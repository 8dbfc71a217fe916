"""CPU tests of the product's host side: world generation parity with the reference,
mesh loading, params, the C-ABI library's exported symbols (no compute without a GPU)."""
import os
import re

import numpy as np
import pytest

import helpers
from conftest import ROOT, golden_cases


@pytest.mark.parametrize("case", golden_cases())
def test_world_generation_is_seed_exact_with_reference(case):
    """reset(seed) builds the same world as the reference's reset(seed): every array that
    the engine consumes (polygons, texcoords, normals, segments, entities, lighting, camera)
    is identical to the fixture extracted from the reference under GL stubs."""
    from miniworld_amd import envs
    from miniworld_amd.scene import scene_from_env
    s0, tr, meta, obs = helpers.load_case(case)
    env = getattr(envs, str(meta["env"]))(host_only=True, **helpers.env_kwargs_of(meta))
    env.reset(seed=int(meta["seed"]))
    sc = scene_from_env(env)
    for k, want in s0.items():
        assert k in sc, k
        assert np.array_equal(np.asarray(sc[k]), np.asarray(want)), f"{case}: {k} differs"


def test_host_only_env_refuses_to_step_or_render():
    from miniworld_amd import envs
    env = envs.Hallway(host_only=True)
    with pytest.raises(RuntimeError):
        env.step(0)


def test_mesh_loader_matches_reference_arrays():
    from miniworld_amd.entity import Ball, Box, Key
    from miniworld_amd.objmesh import ObjMesh
    d = np.load(os.path.join(helpers.GOLDEN, "meshes.npz"))
    for base, name in (("ball", "ball_red"), ("key", "key_blue")):
        m = ObjMesh.get(name)
        for k in ("verts", "norms", "texcs"):
            assert np.array_equal(getattr(m, k), d[f"{base}/{k}"])
        assert np.array_equal(m.max_coords, d[f"{base}/max_coords"])
        assert np.array_equal(m.colors[0, 0], d["kd:" + name].astype(np.float32))
    # Appendix B.4 radii
    assert abs(float(Ball("red", 0.9).radius) - 0.6377) < 1e-4
    assert abs(float(Key("red").radius) - 0.4291) < 1e-4
    assert abs(Box("red", 0.9).radius - 0.6364) < 1e-4 and abs(Box("red").radius - 0.5657) < 1e-4


def test_params_table_and_sampling_stream():
    from miniworld_amd.params import DEFAULT_PARAMS
    assert DEFAULT_PARAMS.get_max("forward_step") == 0.17
    assert DEFAULT_PARAMS.sample(None, "turn_step") == 15
    g1 = np.random.Generator(np.random.PCG64(np.random.SeedSequence(3)))
    g2 = np.random.Generator(np.random.PCG64(np.random.SeedSequence(3)))
    assert DEFAULT_PARAMS.sample(g1, "forward_drift") == g2.uniform(-0.05, 0.05)
    nr = DEFAULT_PARAMS.no_random()
    assert nr.sample(g1, "forward_step") == 0.15


def test_registry_ids():
    from miniworld_amd.envs import ENV_IDS
    for i in ("MiniWorld-Hallway-v0", "MiniWorld-OneRoom-v0", "MiniWorld-Maze-v0", "MiniWorld-PickupObjects-v0"):
        assert i in ENV_IDS


def test_c_abi_library_exports_every_declared_symbol():
    """libmwengine.so loads (no GPU needed) and exports exactly what include/mwengine.h declares."""
    import ctypes
    from miniworld_amd import engine
    engine.build_library()
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    declared = set(re.findall(r"\b(mw_[a-z_0-9]+)\s*\(", header))
    assert declared >= set(engine.EXPORTS)
    lib = ctypes.CDLL(engine.LIB_PATH)
    for sym in sorted(declared):
        assert hasattr(lib, sym), f"{sym} declared in mwengine.h but not exported"
    assert ctypes.sizeof(engine.MwPoly) == 128


def test_engine_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from miniworld_amd import engine, envs
    with pytest.raises(engine.EngineError):
        envs.Hallway()          # no silent CPU fallback


def test_wrappers_semantics_on_host():
    """wrappers.py:7-73: transpose to (C, W, H); float64 greyscale (H, W, 1); stochastic action stream."""
    from miniworld_amd import wrappers
    from miniworld_amd.gymshim import gym

    class Fake(gym.Env):
        observation_space = gym.spaces.Box(0, 255, (60, 80, 3), dtype=np.uint8)
        action_space = gym.spaces.Discrete(8)

        def __init__(self):
            self.rng = np.random.default_rng(0)
            self.last_action = None

        def reset(self, *, seed=None, options=None):
            super().reset(seed=seed)
            return self.rng.integers(0, 256, (60, 80, 3), dtype=np.uint8), {}

        def step(self, action):
            self.last_action = action
            return self.rng.integers(0, 256, (60, 80, 3), dtype=np.uint8), 0.0, False, False, {}

    base = Fake()
    w = wrappers.PyTorchObsWrapper(base)
    assert tuple(w.observation_space.shape) == (3, 80, 60)
    base.rng = np.random.default_rng(5)
    o, _ = w.reset(seed=1)
    base.rng = np.random.default_rng(5)
    raw, _ = base.reset(seed=1)
    assert o.shape == (3, 80, 60) and np.array_equal(o, raw.transpose(2, 1, 0))
    g = wrappers.GreyscaleWrapper(base)
    assert tuple(g.observation_space.shape) == (60, 80, 1)
    base.rng = np.random.default_rng(5)
    og, _ = g.reset(seed=1)
    assert og.dtype == np.float64 and og.shape == (60, 80, 1)
    assert np.array_equal(og[:, :, 0], 0.30 * raw[:, :, 0] + 0.59 * raw[:, :, 1] + 0.11 * raw[:, :, 2])
    s = wrappers.StochasticActionWrapper(base, prob=0.5, random_action=7)
    s.reset(seed=3)
    ref = np.random.Generator(np.random.PCG64(np.random.SeedSequence(3)))
    for a in range(40):
        s.step(a % 3)
        assert base.last_action == ((a % 3) if ref.uniform() < 0.5 else 7)
    s = wrappers.StochasticActionWrapper(base, prob=0.3)
    s.reset(seed=4)
    ref = np.random.Generator(np.random.PCG64(np.random.SeedSequence(4)))
    for a in range(40):
        s.step(2)
        assert base.last_action == (2 if ref.uniform() < 0.3 else ref.integers(0, 6))


def test_pcg64_stream_of_the_engine_is_numpys():
    """MW_RNG_PCG64: the host-side seeding (SeedSequence + pcg_setseq_128_srandom_r) and the draw functions the
    device code inlines (mw_rng.h) reproduce numpy.random.Generator(PCG64(SeedSequence(seed))) — the stream
    gymnasium's np_random(seed) hands the reference (miniworld.py:551): doubles, and bounded integers through
    the buffered 32-bit Lemire path of Generator.integers / Generator.choice, freely interleaved."""
    import ctypes
    from miniworld_amd import engine
    lib = engine.load_library()
    for seed in (0, 1, 7, 4095, 123456789, 2 ** 32 + 17, 2 ** 63 + 3):
        out = np.zeros(64)
        assert lib.mw_pcg64_draws(ctypes.c_uint64(seed), 64, None, out.ctypes.data) == 0
        g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
        assert np.array_equal(out, g.random(64)), seed
        pick = np.random.default_rng(seed)
        bounds = pick.choice([0, 0, 1, 2, 3, 4, 6, 9, 127, 1000003], 400).astype(np.int32)
        out = np.zeros(400)
        assert lib.mw_pcg64_draws(ctypes.c_uint64(seed), 400, bounds.ctypes.data, out.ctypes.data) == 0
        g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
        want = [g.random() if b == 0 else (g.integers(0, b) if i % 2 else g.choice(int(b))) for i, b in enumerate(bounds)]
        assert np.array_equal(out, np.array(want, np.float64)), seed


@pytest.mark.parametrize("case", ["hallway_s0", "hallway_dr_s3", "oneroom_s0", "fourrooms_s0", "maze_s0"])
def test_host_move_and_turn_follow_the_reference_trajectory(case):
    """MiniWorldEnv.move_agent / turn_agent on the host (miniworld.py:620-668): replaying the fixture's actions with
    its per-step parameters reproduces the reference's agent positions and headings bit for bit (float64)."""
    from miniworld_amd import envs
    s0, tr, meta, obs = helpers.load_case(case)
    env = getattr(envs, str(meta["env"]))(host_only=True, **helpers.env_kwargs_of(meta))
    env.reset(seed=int(meta["seed"]))
    assert np.array_equal(np.asarray(env.agent.pos, np.float64), s0["agent_pos"])
    n = 0
    for t, action in enumerate(tr["action"]):
        fwd, drift, turn = float(tr["fwd_step"][t]), float(tr["fwd_drift"][t]), float(tr["turn_step"][t])
        if action == 2:
            env.move_agent(fwd, drift)
        elif action == 3:
            env.move_agent(-fwd, drift)
        elif action == 0:
            env.turn_agent(turn)
        elif action == 1:
            env.turn_agent(-turn)
        else:
            break                                   # pickup / drop / toggle are the engine's
        assert np.array_equal(np.asarray(env.agent.pos, np.float64), tr["pos"][t]), (case, t)
        assert float(env.agent.dir) == float(tr["dir"][t]), (case, t)
        n += 1
        if tr["term"][t] or tr["trunc"][t]:
            break                                   # the fixture resets the episode here
    assert n >= 20


REFERENCE_IDS = [          # miniworld/envs/__init__.py:43-157 (gym.register calls)
    "CollectHealth", "FourRooms", "Hallway", "Maze", "MazeS2", "MazeS3", "MazeS3Fast", "OneRoom", "OneRoomS6",
    "OneRoomS6Fast", "PickupObjects", "PutNext", "RoomObjects", "Sidewalk", "Sign", "ThreeRooms", "TMaze", "TMazeLeft",
    "TMazeRight", "WallGap", "YMaze", "YMazeLeft", "YMazeRight",
]


def test_every_reference_env_id_is_registered_and_batched():
    """Each `MiniWorld-<name>-v0` the reference registers exists as a single-env class, as a gym id and in the
    batched engine's table, and its template world generates on the host."""
    from miniworld_amd import envs
    from miniworld_amd.vec_env import _KIND
    for name in REFERENCE_IDS:
        env_id = f"MiniWorld-{name}-v0"
        assert env_id in _KIND, env_id
        assert envs.ENV_IDS[env_id] == name if hasattr(envs, "ENV_IDS") else hasattr(envs, name)
        cls = getattr(envs, _KIND[env_id][0])
        env = cls(host_only=True)
        env.reset(seed=1)
        assert env.max_episode_steps > 0 and len(env.rooms) >= 1
        # every id is generated, auto-reset and ruled on the device: none is left on the host path
        from miniworld_amd import engine as eng
        assert _KIND[env_id][1] != eng.GEN_NONE, env_id
    fast = envs.MazeS3Fast(host_only=True)
    assert fast.params.get_max("forward_step") == 0.7 and fast.max_episode_steps == 300      # maze.py:75-95
    assert envs.OneRoomS6Fast(host_only=True).max_episode_steps == 50                        # oneroom.py:83-97


def test_placement_programs_compile_for_every_fixed_floorplan_family():
    """genprog.compile_program: rooms, texture tables, ops and the template geometry's metre coordinates (which must
    reproduce the template's own texture coordinates) for each family of the batched table with MW_GEN_PROGRAM."""
    from miniworld_amd import assets, engine as eng, envs, genprog
    from miniworld_amd.scene import scene_from_env
    from miniworld_amd.vec_env import _KIND
    n = 0
    for env_id, (cls, gen, task, _) in _KIND.items():
        if gen != eng.GEN_PROGRAM:
            continue
        t = getattr(envs, cls)(host_only=True)
        t.reset(seed=0)
        sc = scene_from_env(t)
        names = [str(v) for v in sc["tex_names"]]
        for r in t.rooms:
            for nm in (r.wall_tex_name, r.floor_tex_name, r.ceil_tex_name):
                names += [v for v in assets.texture_variants(nm) if v not in names]
        ents = [e for e in t.entities if e is not t.agent]
        ops = genprog.room_objects_ops(0, 1, 2, 0, 6) if cls == "RoomObjects" else genprog.family_ops(t, ents.index, t.rooms.index)
        prog, polys, room, surf, m, segs = genprog.compile_program(t, sc, {v: i for i, v in enumerate(names)},
                                                                   {i: i for i in range(len(sc["mesh_names"]))}, ops)
        assert prog.n_rooms == len(t.rooms) and prog.n_ents == len(ents) and prog.n_ops == len(ops)
        assert abs(prog.rooms[prog.n_rooms - 1].cdf - 1.0) < 1e-12
        assert (room >= 0).sum() >= 5 and len(polys) == len(sc["polys_nv"]) and len(segs) == len(sc["wall_segs"])
        n += 1
    assert n == 14


def test_rooms_with_more_than_four_corners_are_the_references():
    """Room accepts any outline (miniworld.py:127-176); floor and ceiling are then GL_POLYGONs of that many vertices, which
    the driver draws as the triangles (i, i + 1, 0).  tests/golden/gl_ngon_*.npz are the reference's own frames of a hexagonal
    and a heptagonal room on llvmpipe (tools/gen_gl_fixtures.py: EXTRA; the pixel tests take them like every other fixture);
    here: the host classes build that world from the same seed, and the scene the engine gets — one triangle polygon per
    fan triangle — is the fixture's."""
    from miniworld_amd.entity import Box
    from miniworld_amd.miniworld import MiniWorldEnv
    from miniworld_amd.scene import scene_from_env

    class NGonRooms(MiniWorldEnv):
        def __init__(self, **kw):
            super().__init__(max_episode_steps=200, **kw)

        def _gen_world(self):
            def ring(cx, cz, r, n, t0):
                return np.array([[cx + r * np.cos(t0 + 2 * np.pi * k / n), cz - r * np.sin(t0 + 2 * np.pi * k / n)] for k in range(n)])
            self.add_room(outline=ring(0.0, 0.0, 4.5, 6, 0.3))
            self.add_room(outline=ring(12.0, 1.0, 3.5, 7, 1.1), wall_tex="brick_wall", floor_tex="asphalt", no_ceiling=True)
            self.box = self.place_entity(Box(color="red"), room=self.rooms[0])
            self.box2 = self.place_entity(Box(color="blue", size=0.5), room=self.rooms[1])
            self.place_agent(room=self.rooms[0])

    env = NGonRooms(host_only=True)
    env.reset(seed=0)
    sc = scene_from_env(env)
    d = np.load(os.path.join(helpers.GOLDEN, "gl_ngon_s0.npz"))
    assert sc["polys_v"].shape[0] == 26        # 4 + 4 fan triangles + 6 walls; 5 fan triangles + 7 walls
    for k in ("polys_v", "polys_uv", "polys_n", "polys_nv", "polys_tex", "polys_rgb", "agent_pos", "agent_dir", "ents_pos", "ents_dir",
              "ents_size", "ents_color", "wall_segs"):
        assert np.array_equal(np.asarray(sc[k]), d["gl/0/scene/" + k]), k


def test_footprint_record_operands_reproduce_the_8_8_lerp_for_every_input():
    """The engine's texture footprint records hold, per channel and texel pair, A = 256 a + 128 and D = (b - a) mod 2^16
    (mw_assets.h::build_pyramid); the raster kernel's x lerp is one packed 16-bit multiply-add and a shift,
    (A + w D) mod 2^16 >> 8 (mw_raster_common.h::lerp8_ad).  Exhaustively over a, b, w in 0 .. 255 that is llvmpipe's
    a + ((w (b - a) + 128) >> 8) — and so is the three-instruction form of the other lerps, (a (256 - w) + (b w + 128)) >> 8,
    whose sums stay below 2^16."""
    a = np.arange(256, dtype=np.int64)[:, None, None]
    b = np.arange(256, dtype=np.int64)[None, :, None]
    w = np.arange(256, dtype=np.int64)[None, None, :]
    want = a + ((w * (b - a) + 128) >> 8)                     # arithmetic shift: mwgl::lerp8
    A, D = (a * 256 + 128) & 0xFFFF, (b - a) & 0xFFFF
    got = ((A + D * w) & 0xFFFF) >> 8
    assert np.array_equal(got, np.broadcast_to(want, got.shape))
    s1 = b * w + 128
    s2 = a * (256 - w) + s1
    assert s1.max() < 65536 and s2.max() < 65536
    assert np.array_equal(s2 >> 8, np.broadcast_to(want, got.shape))
    assert want.min() >= 0 and want.max() <= 255


def test_register_bitonic_network_of_the_visiting_order_sorts():
    """Big scenes' geometry kernel sorts up to 512 (depth bound << 16 | list index) keys with a bitonic network whose keys
    live in registers — key i = 64 r + lane in register r of the lane — so that a stage is either a lane shuffle
    (partner lane ^ j) or a register swap (partner r ^ (j / 64)); K2's early exit relies on the result being ascending.
    This is mw_geom.hip::sort_store_keys<R> statement for statement (the direction of every compare-exchange is the part
    that is easy to get wrong), run for R = 1, 2, 4, 8 and list lengths that leave padding."""
    def network_sort(keys, R):
        n = len(keys)
        x = np.full((R, 64), 0xFFFFFFFF, np.uint64)
        x.reshape(-1)[:n] = keys                                  # x[r][lane] = keys[64 r + lane]
        lanes = np.arange(64)
        k = 2
        while k <= 64 * R:
            j = k >> 1
            while j > 0:
                if j >= 64:                                         # partners in two registers of the same lane
                    jj = j >> 6
                    for r in range(R):
                        if r & jj:
                            continue
                        up = ((64 * r) & k) == 0
                        lo, hi = np.minimum(x[r], x[r ^ jj]), np.maximum(x[r], x[r ^ jj])
                        x[r], x[r ^ jj] = (lo, hi) if up else (hi, lo)
                else:                                               # partners in two lanes, the same register
                    for r in range(R):
                        y = x[r][lanes ^ j]
                        up = (((64 * r) | lanes) & k) == 0
                        keep_min = ((lanes & j) == 0) == up
                        x[r] = np.where(keep_min, np.minimum(x[r], y), np.maximum(x[r], y))
                j >>= 1
            k <<= 1
        return x.reshape(-1)[:n]

    rng = np.random.default_rng(0)
    for R in (1, 2, 4, 8):
        for n in [64 * R, 64 * R - 1, 32 * R + 1] + [int(v) for v in rng.integers(32 * R + 1, 64 * R + 1, 12)]:
            keys = (rng.integers(0, 65536, n).astype(np.uint64) << 16) | np.arange(n, dtype=np.uint64)
            assert np.array_equal(network_sort(keys, R), np.sort(keys)), (R, n)

