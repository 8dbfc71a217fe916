"""The launch shapes that only large batches reach, at small batches (mw_debug_set_launch_shape) — and the frame plan at the two batch
sizes where its form changes, which no small batch can stand in for.

The launch policy gives a wavefront of the tile kernels more than one tile, and a persistent worker of the mesh path more than one item,
only when the batch is large (mw_policy.h: pick_waves_per_env; mw_engine.h: MeshPath's worker counts).  The loops that then run a second
time — the tx / ty walk across tile rows, the groups of 64 / nvis tiles classified in one pass with lane gi's masks, the restaging of a
workgroup's vertex table and queues for its next entity, a tile wavefront's next listed tile — are run here on the fixtures and the
synthetic capacity scenes of tests/test_gpu_display_list_limits.py with the shape set by hand.  Every comparison is np.array_equal with
pyoracle.render of the same scene, RGB and depth map; mw_check is clean after every engine; the path, the list lengths, a mesh in view,
a triangle on the slow path are asserted, never assumed.

The plan (mw_frame_plan.h): 65535 envs are the largest ordered plan — a 16-bit class count can read 0xFFFF beside three others in its
64-bit word —, 65536 the smallest unordered one.  The oracle cannot render that many frames, so the batch is K-periodic by construction
(env i starts in state i % K and takes the actions of residue i % K) and is checked to be: on the device, every frame and source byte
equals that of env i % K; envs 0 .. K - 1 are held to the oracle.  (frame_plans' own limit, 2^24 envs, is out of a test's reach.)"""
import functools
import time

import numpy as np
import pytest

import helpers
import test_display_list_limits_cpu as cpu
import test_gpu_display_list_limits as lim
import test_gpu_plan_order as tpo

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ a, b: tile runs on the capacity scenes

@pytest.mark.parametrize("wpe", [1, 3, 5, 15, 25])
@pytest.mark.parametrize("config", ["tile-depth", "tile-rgb"])
@pytest.mark.parametrize("which", ["lengths", "crowded", "overlaps"])
def test_small_scene_tile_runs_of_75_to_3_tiles(which, config, wpe, monkeypatch):
    """80 x 60 is 5 x 15 tiles: 75, 25, 15, 5 and 3 tiles per wavefront (1 is what every other test runs).  With the whole frame in one
    run, display lists of 1 .. 32 triangles are classified in groups of 64, 32, 21, 16, 12, ... 2 tiles, most of which leave a short last
    group and all of which straddle a tile row; 33 is the first length that leaves the pairs branch (draw_and_compare holds the engine's
    lengths to the pinned ones)."""
    assert set(range(1, 34)) <= set(cpu.LENGTHS)
    lim.run_config(which, config, monkeypatch, shape={"waves_per_env": wpe})


@pytest.mark.parametrize("wpe", [1, 5, 25])
@pytest.mark.parametrize("config", ["big-depth", "big-rgb"])
@pytest.mark.parametrize("which", ["lengths", "crowded", "overlaps"])
def test_big_scene_tile_runs(which, config, wpe, monkeypatch):
    """max_visible = 65: a visiting order, records read in place"""
    lim.run_config(which, config, monkeypatch, shape={"waves_per_env": wpe})


# ------------------------------------------------------------------ c: the other instantiations, on fixtures

@functools.lru_cache(maxsize=None)
def fixture_frames(case, width=80, height=60):
    """(s0, the scenes of the fixture's first three frames, the oracle's frames of them: rendered once, never written to)"""
    import pyoracle
    s0, tr, meta, obs = helpers.load_case(case)
    scenes = [helpers.frame_scene(s0, obs[f]) for f in sorted(obs)[:3]]
    meshes = helpers.golden_meshes(s0)
    return s0, scenes, [pyoracle.render(sc, width=width, height=height, meshes=meshes) for sc in scenes]


def without_entities(scene, which=None):
    """the scene with the entities of `which` (default: every mesh entity) taken out"""
    sc = dict(scene)
    gone = np.asarray(scene["ents_mesh"]) >= 0 if which is None else np.asarray(which)
    sc["ents_kind"] = np.where(gone, 0, np.asarray(scene["ents_kind"]))
    return sc


def draw_fixture(case, shape, want_path, width=80, height=60, with_depth=True, layout="hwc"):
    """The fixture's first three frames under a launch shape against the oracle; returns how many meshes the engine holds."""
    import torch
    from miniworld_amd import engine as E
    from test_gpu_obs_sizes import _grey
    s0, scenes, want = fixture_frames(case, width, height)
    eng = helpers.make_engine_for_scene(s0, len(scenes), width=width, height=height)
    eng.debug_set_launch_shape(**shape)
    if layout != "hwc":
        eng.set_obs_layout({"cwh": E.OBS_CWH_U8, "grey": E.OBS_GREY_F64}[layout])
    eng.set_state(helpers.scene_state_arrays(scenes))
    obs = eng.obs_buffer()
    depth = torch.zeros((len(scenes), height, width, 1), dtype=torch.float32, device="cuda") if with_depth else None
    eng.render(obs, depth)
    eng.check()
    path, n_meshes = eng.raster_path(), len(eng._test_mesh_map)
    obs = obs.cpu().numpy()
    depth = depth.cpu().numpy() if with_depth else None
    eng.close()
    assert path == want_path, path
    for i, w in enumerate(want):
        frame = {"hwc": w["rgb"], "cwh": w["rgb"].transpose(2, 1, 0), "grey": _grey(w["rgb"])[..., None]}[layout]
        assert obs[i].shape == frame.shape and obs[i].dtype == frame.dtype
        assert np.array_equal(obs[i], frame), (case, shape, layout, f"frame {i}: {np.count_nonzero(obs[i] != frame)} values differ")
        if with_depth:
            assert np.array_equal(depth[i], w["depth"]), (case, shape, f"frame {i}: {np.count_nonzero(depth[i] != w['depth'])} depths differ")
    return n_meshes


@pytest.mark.parametrize("wpe", [1, 5, 25])
@pytest.mark.parametrize("with_depth", [True, False])
def test_the_maze_in_runs_of_tiles(with_depth, wpe):
    """a big scene of its own: 510 polygons, the visiting order long"""
    from miniworld_amd import engine as E
    draw_fixture("maze_s0", {"waves_per_env": wpe}, E.PATH_TILE, with_depth=with_depth)


@pytest.mark.parametrize("wpe", [1, 5])
@pytest.mark.parametrize("layout", ["cwh", "grey"])
def test_the_wrap_kernels_in_runs_of_tiles(layout, wpe, monkeypatch):
    """another output layout on the tile path: the general instantiation"""
    from miniworld_amd import engine as E
    monkeypatch.setenv("MW_K2Q", "0")
    draw_fixture("hallway_s0", {"waves_per_env": wpe}, E.PATH_TILE, with_depth=False, layout=layout)


@pytest.mark.parametrize("case,size,wpe", [("hallway_s0", (72, 58), 1), ("hallway_s0", (72, 58), 15),
                                           ("hallway_s0", (84, 84), 1), ("hallway_s0", (84, 84), 14), ("hallway_s0", (84, 84), 126),
                                           ("maze_s0", (84, 84), 1), ("maze_s0", (84, 84), 14)])
@pytest.mark.parametrize("with_depth", [True, False])
def test_the_ragged_kernels_in_runs_of_tiles(with_depth, case, size, wpe):
    """72 x 58 is 5 x 15 = 75 tiles with padding on both sides, 84 x 84 is 6 x 21 = 126 (the policy's 9 tiles per wavefront at 4096 envs
    are waves_per_env = 14); the Maze takes the big-scene ragged kernel"""
    from miniworld_amd import engine as E
    draw_fixture(case, {"waves_per_env": wpe}, E.PATH_TILE, width=size[0], height=size[1], with_depth=with_depth)


@pytest.mark.parametrize("wpe", [1, 5])
@pytest.mark.parametrize("with_depth", [True, False])
def test_the_mesh_aware_first_part_in_runs_of_tiles(with_depth, wpe, monkeypatch):
    """PickupObjects with MW_K2Q=0: the tile kernel draws every tile no mesh can touch (mw_raster_nomesh, _depth) in runs, the tiles inside
    a mesh rectangle skipped on the way"""
    import pyoracle
    from miniworld_amd import engine as E
    monkeypatch.setenv("MW_K2Q", "0")
    s0, scenes, want = fixture_frames("pickup_s0")
    meshes = helpers.golden_meshes(s0)
    shown = [int(np.count_nonzero(w["rgb"] != pyoracle.render(without_entities(sc), meshes=meshes)["rgb"])) for sc, w in zip(scenes, want)]
    assert all(shown), ("a frame without a mesh entity in view", shown)
    assert draw_fixture("pickup_s0", {"waves_per_env": wpe}, E.PATH_TILE, with_depth=with_depth) > 0, "no mesh uploaded"


def test_the_list_forms_in_one_run_of_tiles(monkeypatch):
    """A same-step auto-reset step with final observations under MW_K2Q=0, every frame one wavefront's run of 75 tiles: the first pass
    (the plain kernels: terminal frames) and the list pass over the finished envs (the *_sub kernels: their new worlds' frames).  After
    every step each env's frame is the oracle's of the state the device holds, each finished env's final frame the oracle's of the
    terminal state — which a twin without auto-reset holds after the same step."""
    import pyoracle
    import torch
    from miniworld_amd import engine as E
    from miniworld_amd.vec_env import MiniWorldVecEnv
    from test_gpu_final_obs import _short_episodes
    monkeypatch.setenv("MW_K2Q", "0")
    _short_episodes(monkeypatch, "TMaze", 4)
    n = 8
    A = MiniWorldVecEnv("MiniWorld-TMaze-v0", n, seed=60, want_depth=True, final_obs=True)
    C = MiniWorldVecEnv("MiniWorld-TMaze-v0", n, seed=60, want_depth=True, autoreset=False)
    A.engine.debug_set_launch_shape(waves_per_env=1)
    A.reset()
    C.reset()
    g = torch.Generator(device="cuda").manual_seed(1)
    finished = 0
    for t in range(6):
        act = torch.randint(0, 3, (n,), generator=g, device="cuda", dtype=torch.int32)
        _, _, term, trunc = A.step(act)
        C.step(act)
        done = (term | trunc).bool().cpu().numpy()
        sa, sc = A.engine.get_state(), C.engine.get_state()
        obs, depth = A.obs.cpu().numpy(), A.depth.cpu().numpy()
        for i in range(n):
            want = pyoracle.render(helpers.scene_of_vec_env(A, sa, i))
            assert np.array_equal(obs[i], want["rgb"]) and np.array_equal(depth[i], want["depth"]), (t, i, bool(done[i]))
        for i in np.flatnonzero(done):
            want = pyoracle.render(helpers.scene_of_vec_env(C, sc, i))
            assert np.array_equal(A.final_obs[i].cpu().numpy(), want["rgb"]), (t, i)
            assert np.array_equal(A.final_depth[i].cpu().numpy(), want["depth"]), (t, i)
            finished += 1
        if done.any():
            C.engine.reset(done.astype(np.uint8), None)
    assert finished >= n and A.engine.raster_path() == E.PATH_TILE
    A.engine.check()
    A.close()
    C.close()


# ------------------------------------------------------------------ d: persistent workers of the mesh path

MESH_ENVS = 16


def crack_the_balls(s0, meshes):
    """test_gpu_render_parity's cracked balls: every large mesh gets more distinct positions than a vertex table holds; returns their ids"""
    rng = np.random.default_rng(11)
    cracked = []
    for i, name in enumerate([str(m) for m in s0["mesh_names"]]):
        m = meshes[name]
        if len(m["verts"]) < 2000:
            continue
        m["verts"] = (m["verts"] + rng.uniform(-2e-3, 2e-3, m["verts"].shape)).astype(np.float32)
        assert len(np.unique(m["verts"].reshape(-1, 3), axis=0)) > 3584
        cracked.append(i)
    return cracked


@functools.lru_cache(maxsize=None)
def mesh_batches(case, cracked=False):
    """(s0, meshes, cracked mesh ids, [2 frames][MESH_ENVS scenes], [2][MESH_ENVS] the oracle's frames).  The scenes are the fixture's
    frames with a mesh entity in view — the oracle's frame differs from its frame of the scene without them —, dealt so that the two envs
    of every class env % 8 show different ones; the second frame deals them one further."""
    import pyoracle
    s0, tr, meta, obs = helpers.load_case(case)
    meshes = helpers.golden_meshes(s0)
    ids = crack_the_balls(s0, meshes) if cracked else []
    base, want = [], []
    for f in sorted(obs):
        sc = helpers.frame_scene(s0, obs[f])
        w = pyoracle.render(sc, meshes=meshes)
        if np.count_nonzero(w["rgb"] != pyoracle.render(without_entities(sc), meshes=meshes)["rgb"]):
            base.append(sc)
            want.append(w)
    k = len(base)
    assert k >= 2, (case, "fewer than two frames with a mesh entity in view")
    if cracked:
        # a cracked ball and an intact key in view of one env: its class's workgroup draws a mesh without a table and one with
        both = 0
        for sc, w in zip(base, want):
            is_cracked = np.isin(np.asarray(sc["ents_mesh"]), ids)
            is_intact = (np.asarray(sc["ents_mesh"]) >= 0) & ~is_cracked
            both += all(np.count_nonzero(w["rgb"] != pyoracle.render(without_entities(sc, which), meshes=meshes)["rgb"]) for which in (is_cracked, is_intact))
        assert ids and both, (case, "no frame shows a cracked ball beside an intact mesh")
    deal = [[(i + (i // 8) * (k - 1) + frame) % k for i in range(MESH_ENVS)] for frame in (0, 1)]
    assert all(d[r] != d[r + 8] for d in deal for r in range(8))
    return s0, meshes, ids, [[base[j] for j in d] for d in deal], [[want[j] for j in d] for d in deal]


def draw_mesh_batches(case, want_path, with_depth, shape, cracked=False):
    """Two frames of one engine (the work lists' counters swap sides: the second frame starts from what the first one's kernel zeroed)
    against the oracle; returns the pixels of the first frame that hold a fragment of the slow path."""
    import torch
    from miniworld_amd.engine import _stream_ptr
    s0, meshes, ids, batches, wants = mesh_batches(case, cracked)
    eng = helpers.make_engine_for_scene(s0, MESH_ENVS)
    for i in ids:
        m = meshes[str(s0["mesh_names"][i])]
        eng.upload_mesh(eng._test_mesh_map[i], m["verts"], m["norms"], m["texcs"], m["colors"], -1)
    eng.debug_set_launch_shape(**shape)
    slow = None
    for frame, (scenes, want) in enumerate(zip(batches, wants)):
        eng.set_state(helpers.scene_state_arrays(scenes))
        rgb = torch.zeros((MESH_ENVS, 60, 80, 3), dtype=torch.uint8, device="cuda")
        depth = torch.zeros((MESH_ENVS, 60, 80, 1), dtype=torch.float32, device="cuda") if with_depth else None
        eng.render(rgb, depth)
        eng.check()
        assert eng.raster_path() == want_path, eng.raster_path()
        if slow is None:
            heads = np.zeros((MESH_ENVS, 60, 80), np.uint32)
            assert eng.lib.mw_debug_get_slow_heads(eng.h, heads.ctypes.data, _stream_ptr(eng.device)) == 0
            slow = int(np.count_nonzero(heads))         # (a new engine's heads are zero)
        rgb = rgb.cpu().numpy()
        depth = depth.cpu().numpy() if with_depth else None
        for i, w in enumerate(want):
            tag = (case, shape, f"frame {frame}, env {i}")
            assert np.array_equal(rgb[i], w["rgb"]), tag + (f"{np.count_nonzero(rgb[i] != w['rgb'])} RGB values differ",)
            if with_depth:
                assert np.array_equal(depth[i], w["depth"]), tag + (f"{np.count_nonzero(depth[i] != w['depth'])} depths differ",)
    eng.close()
    return slow


# 8 workers of a kind: one per class env % 8, and every class holds two envs with a mesh entity in view — each entity workgroup and each
# tile wavefront that has work takes at least two items; one slow wavefront takes every item there is.  24: three workers of a class race
# for its cursor or stride over its list.
WORKERS = {"8-8-1": {"ent_blocks": 8, "mesh_tile_waves": 8, "slow_waves": 1}, "24-24-2": {"ent_blocks": 24, "mesh_tile_waves": 24, "slow_waves": 2}}
MESH_PATHS = {"quad-mesh": ({}, "PATH_QUAD_MESH"), "tile": ({"MW_K2Q": "0"}, "PATH_TILE")}


@pytest.mark.parametrize("workers", WORKERS)
@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("path", MESH_PATHS)
@pytest.mark.parametrize("case", ["pickup_s0", "pickup_fwd_s2", "pickup_dr_s1"])
def test_persistent_workers_take_several_items(case, path, with_depth, workers, monkeypatch):
    from miniworld_amd import engine as E
    env, want_path = MESH_PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    slow = draw_mesh_batches(case, getattr(E, want_path), with_depth, WORKERS[workers])
    if case == "pickup_fwd_s2":
        assert slow > 0, "no mesh triangle across a frustum plane: the slow kernel's loop saw no item"


@pytest.mark.parametrize("workers", WORKERS)
@pytest.mark.parametrize("path", MESH_PATHS)
def test_a_workgroup_draws_a_mesh_without_a_table_and_then_one_with(path, workers, monkeypatch):
    """cracked balls (no vertex table: every triangle through the vertex stage by itself, then the loop's `continue`) beside intact keys
    (the table restaged) in the lists of one workgroup"""
    from miniworld_amd import engine as E
    env, want_path = MESH_PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    draw_mesh_batches("pickup_s0", getattr(E, want_path), True, WORKERS[workers], cracked=True)


# ------------------------------------------------------------------ e: what the setter refuses

def test_a_refused_shape_changes_nothing(monkeypatch):
    import torch
    from miniworld_amd import engine as E
    monkeypatch.setenv("MW_K2Q", "0")
    s0, scenes, want = fixture_frames("pickup_s0")
    eng = helpers.make_engine_for_scene(s0, len(scenes))
    eng.set_state(helpers.scene_state_arrays(scenes))
    eng.debug_set_launch_shape(waves_per_env=5, mesh_tile_waves=8, ent_blocks=8, slow_waves=1)

    def frame():
        rgb = torch.zeros((len(scenes), 60, 80, 3), dtype=torch.uint8, device="cuda")
        depth = torch.zeros((len(scenes), 60, 80, 1), dtype=torch.float32, device="cuda")
        eng.render(rgb, depth)
        eng.check()
        return rgb.cpu().numpy(), depth.cpu().numpy()

    before = frame()
    refused = [dict(waves_per_env=7), dict(waves_per_env=150), dict(mesh_tile_waves=7), dict(ent_blocks=7), dict(ent_blocks=1), dict(slow_waves=-1),
               dict(waves_per_env=-1), dict(mesh_tile_waves=-8), dict(ent_blocks=-8),
               dict(waves_per_env=25, mesh_tile_waves=64, ent_blocks=7), dict(waves_per_env=7, slow_waves=4)]
    for shape in refused:
        with pytest.raises(E.EngineError, match="mw_debug_set_launch_shape"):
            eng.debug_set_launch_shape(**shape)
    assert eng.lib.mw_debug_set_launch_shape(None, 1, 0, 0, 0) != 0
    after = frame()
    eng.debug_set_launch_shape()            # (all zero: every value stays)
    again = frame()
    eng.close()
    for got in (before, after, again):
        for i, w in enumerate(want):
            assert np.array_equal(got[0][i], w["rgb"]) and np.array_equal(got[1][i], w["depth"]), i
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ------------------------------------------------------------------ the frame plan at 65535 and 65536 envs

PLAN_K, PLAN_STEPS, PLAN_SLOTS = 16, 6, 2


@functools.lru_cache(maxsize=None)
def plan_states():
    """(s0, PLAN_K scenes along the Hallway fixture's trajectory, the step parameters the reference drew: one row)"""
    s0, tr, meta, obs = helpers.load_case("hallway_s0")
    first = {}          # distinct poses -> the step that reached them first (the agent also turns back and stands at walls)
    for t in range(len(tr["dir"])):
        first.setdefault(tr["pos"][t].tobytes() + tr["dir"][t].tobytes(), t)
    assert not tr["term"].any() and not tr["trunc"].any()
    scenes = []
    for t in sorted(first.values())[::4][:PLAN_K]:      # (display lists of 24 down to 2 triangles: several cost classes)
        sc = dict(s0)
        sc["agent_pos"], sc["agent_dir"] = tr["pos"][t], tr["dir"][t]
        sc["ents_pos"], sc["ents_dir"] = tr["ents_pos"][t], tr["ents_dir"][t]
        scenes.append(sc)
    assert len({sc["agent_pos"].tobytes() + np.float64(sc["agent_dir"]).tobytes() for sc in scenes}) == PLAN_K
    return s0, scenes, np.array([tr["fwd_step"][0], tr["fwd_drift"][0], tr["turn_step"][0]])


@pytest.mark.parametrize("n", [65535, 65536])
def test_the_plan_at_the_largest_ordered_and_the_smallest_unordered_batch(n):
    import pyoracle
    import torch
    s0, scenes, params = plan_states()
    K, ordered = PLAN_K, n <= 0xFFFF
    residue = np.arange(n) % K
    residue_d = torch.as_tensor(residue, device="cuda")
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    eng = helpers.make_engine_for_scene(s0, n)
    assert eng.set_frame_reuse(True) and eng.set_frame_cache(PLAN_SLOTS) == PLAN_SLOTS
    eng.set_step_params(np.tile(params, (n, 1)))
    rgb = torch.zeros((n, 60, 80, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t_create = time.perf_counter() - t0
    held = free0 - torch.cuda.mem_get_info()[0]

    def step(actions, tag):
        """one step; the block against the source bytes; returns (source bytes, the block's classes or envs along the draw list)"""
        eng.step(torch.as_tensor(actions, dtype=torch.int32, device="cuda"), rgb)
        src = eng.get_frame_source().cpu().numpy()
        return src, tpo._check_plan(tag, eng, src, ordered=ordered, slots=PLAN_SLOTS)

    def set_states(of_env):
        one = helpers.scene_state_arrays(scenes)
        eng.set_state({k: np.ascontiguousarray(v[of_env]) for k, v in one.items()})

    # every env in one state: the step behind set_state draws every env, all of one cost class
    set_states(np.zeros(n, np.int64))
    src, _ = step(np.full(n, tpo.L), (n, "one state"))
    assert (src == 0).all()
    p = eng.get_frame_plan()
    if ordered:
        assert sorted(p["class_counts"]) == [0] * 7 + [0xFFFF], p["class_counts"]       # (its three neighbours in the word read 0)
        packed = [int(p["block"][32]) | int(p["block"][33]) << 32, int(p["block"][64]) | int(p["block"][65]) << 32]
        assert sorted(packed)[0] == 0 and sorted(packed)[1] in [0xFFFF << s for s in (0, 16, 32, 48)], [hex(w) for w in packed]
    else:
        assert p["n_draw"] == n and p["classes"] == 0
    assert torch.equal(rgb, rgb[:1].expand_as(rgb))

    # K states, the script of tests/test_gpu_plan_order.py per residue
    set_states(residue)
    script = tpo._script(K, 33)[:PLAN_STEPS]
    models = [tpo._Model(PLAN_SLOTS) for _ in range(K)]
    rendered, most_classes, mixed = {}, 0, False
    for t in range(PLAN_STEPS):
        tag = (n, "step", t)
        src, along = step(script[t][residue], tag)
        # K-periodic on the device: frames and source bytes
        assert torch.equal(rgb, rgb[residue_d]), (tag, "the frames are not periodic")
        assert np.array_equal(src, src[residue]), (tag, "the source bytes are not periodic")
        # envs 0 .. K - 1: the oracle's frames, the host model's source bytes
        st = eng.get_state(0, K)
        clean = eng.get_frame_clean().cpu().numpy()[:K].astype(bool)
        got = rgb[:K].cpu().numpy()
        for i in range(K):
            sc = dict(s0)
            sc["agent_pos"], sc["agent_dir"] = st["agent_pos"][i], st["agent_dir"][i]
            sc["ents_pos"], sc["ents_dir"], sc["ents_kind"] = st["ent_pos"][i, :1], st["ent_dir"][i, :1], st["ent_kind"][i, :1]
            key = tpo._state_bytes(st, i)
            if key not in rendered:
                rendered[key] = pyoracle.render(sc)["rgb"]
            assert np.array_equal(got[i], rendered[key]), (tag, "env", i, "source", int(src[i]))
            pose = np.ascontiguousarray(st["agent_pos"][i], np.float64).tobytes() + np.float64(st["agent_dir"][i]).tobytes()
            assert models[i].step(pose, bool(clean[i]), False)[0] == src[i], (tag, "env", i, "source", int(src[i]))
        assert (st["carrying"] < 0).all()
        if ordered:
            most_classes = max(most_classes, len(set(along.tolist())))
        mixed |= bool((src == 0).any() and (src == 1).any() and (src >= 2).any())
    eng.check()
    eng.close()
    assert mixed, "no step in which drawn, clean and copied envs share the launch"
    if ordered:
        assert most_classes >= 2, "no step whose draw list holds two cost classes"
    print(f"\n[{n} envs] engine + frame buffer made in {t_create:.2f} s, {held / 2 ** 20:.0f} MiB of device memory held, test {time.perf_counter() - t0:.2f} s")
