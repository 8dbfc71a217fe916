"""Rotations by large angles on the GPU against the oracle, bit for bit.

Every Box, MeshEnt and ImageFrame is drawn through glRotatef, i.e. glibc's sinf / cosf of the entity's heading
(mw_glmath.h sincosf_glibc).  Headings are not wrapped: a carried entity takes the agent's heading on every turn, so an
agent that keeps turning carries a box at hundreds of radians, and mw_set_state accepts any angle.  glibc reduces
|x| < 120 one way and larger arguments with a table of 4 / pi; here every kernel that draws an entity gets angles on both
sides of that line and far beyond it, one angle per env in one batch, so that one launch mixes lanes of both reductions.
The agent's own heading stays below 1e6, the domain of its f64 sin / cos (mwengine.h, mw_set_state).
"""
import math

import numpy as np
import pytest

import helpers
from test_oracle_vs_reference_gl import load_gl

pytestmark = pytest.mark.gpu

AGENT_ANGLES = [119.99, -119.99, 120.0, -120.0, 125.0, 150.0, 201.06, 250.0, 1e3, 1e5]
ENTITY_ONLY_ANGLES = [1e7, 1e30, -1e30]          # entities only: the agent's heading stays inside its domain


def carry_pos(sc, k, agent_pos, agent_dir):
    """MiniWorldEnv._get_carry_pos (miniworld.py:606-618) for entity k of the scene."""
    dist = float(sc["agent_radius"]) + float(sc["ents_radius"][k]) + float(sc["max_forward_step"])
    pos = np.asarray(agent_pos, np.float64) + np.array([math.cos(agent_dir), 0.0, -math.sin(agent_dir)]) * 1.05 * dist
    pos[1] += max(float(sc["cam_height"]) - float(sc["ents_height"][k]) - 0.3, 0.0)
    return pos


def angle_scenes(s0, carried):
    """One scene per angle: every entity's heading is the angle; the agent stands where it stands in s0, turned to the
    angle (kept at s0's heading for the entity-only angles), carrying entity `carried` (None: nothing) in front of it."""
    scenes = []
    for a in AGENT_ANGLES + ENTITY_ONLY_ANGLES:
        sc = dict(s0)
        agent_dir = a if abs(a) < 1e6 else float(s0["agent_dir"])
        sc["agent_dir"] = np.float64(agent_dir)
        pos = np.array(s0["ents_pos"], np.float64).copy()
        if carried is not None:
            pos[carried] = carry_pos(s0, carried, s0["agent_pos"], agent_dir)
            sc["agent_carrying"] = np.int32(carried)
        sc["ents_pos"] = pos
        sc["ents_dir"] = np.full(len(s0["ents_kind"]), a, np.float64)
        scenes.append(sc)
    return scenes


def render_and_compare(scenes, meshes, msaa, label, path=None, size=(80, 60), views=False):
    """The engine's frames of the batch (and with views: its top views and 800 x 600 render_view frames) == the oracle's."""
    import torch
    import pyoracle
    W, H = size
    s0 = scenes[0]
    eng = helpers.make_engine_for_scene(s0, len(scenes), agent_radius=float(s0["agent_radius"]), msaa=msaa, width=W, height=H)
    try:
        eng.set_state(helpers.scene_state_arrays(scenes))
        rgb = torch.zeros((len(scenes), H, W, 3), dtype=torch.uint8, device="cuda")
        depth = torch.zeros((len(scenes), H, W, 1), dtype=torch.float32, device="cuda")
        eng.render(rgb, depth)
        eng.check()
        got_path = eng.raster_path()
        if path is not None:
            assert got_path in path, (label, got_path)
        rgb, depth = rgb.cpu().numpy(), depth.cpu().numpy()
        for i, sc in enumerate(scenes):
            want = pyoracle.render(sc, width=W, height=H, nsamples=msaa, meshes=meshes)
            a = float(sc["ents_dir"][0])
            assert np.array_equal(depth[i], want["depth"]), f"{label}, angle {a}: depth differs"
            assert np.array_equal(rgb[i], want["rgb"]), f"{label}, angle {a}: {np.count_nonzero(rgb[i] != want['rgb'])} RGB values differ"
        if views:
            top = torch.zeros((len(scenes), H, W, 3), dtype=torch.uint8, device="cuda")
            eng.render_top(top, None, True)
            eng.check()
            top = top.cpu().numpy()
            for i, sc in enumerate(scenes):
                want = pyoracle.render(sc, width=W, height=H, nsamples=msaa, meshes=meshes, view="top", render_agent=True)
                assert np.array_equal(top[i], want["rgb"]), f"{label}, angle {float(sc['ents_dir'][0])}: top view differs"
            for i in (0, 4, 7, len(scenes) - 1):
                out = eng.render_view(i, 800, 600, msaa=msaa).cpu().numpy()
                eng.check()
                want = pyoracle.render(scenes[i], width=800, height=600, nsamples=msaa, meshes=meshes)
                assert np.array_equal(out, want["rgb"]), f"{label}, angle {float(scenes[i]['ents_dir'][0])}: 800x600 view differs"
        return got_path
    finally:
        eng.close()


def first_scene(case):
    frames = load_gl(case)
    return frames[sorted(frames)[0]][0]


def putnext_carried():
    s0 = first_scene("putnext_s0")
    return s0, [k for k in range(len(s0["ents_kind"])) if not s0["ents_static"][k]][0]


@pytest.mark.parametrize("msaa,env,label", [
    (8, {}, "quad kernel (K2Q), 8 samples"),
    (8, {"MW_K2Q": "0"}, "tile kernels, 8 samples"),
    (4, {}, "quad kernel, 4 samples"),
    (4, {"MW_GENERIC_RASTER": "1"}, "generic kernel, 4 samples"),
    (1, {}, "1 sample"),
])
def test_carried_box_at_large_angles(msaa, env, label, monkeypatch):
    """PutNext: a carried box (at the agent's heading) and the other boxes at angles around 120 rad and far beyond;
    at 8 samples also the top view and render() at 800 x 600."""
    from miniworld_amd import engine as E
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s0, carried = putnext_carried()
    want_path = {"MW_K2Q": (E.PATH_TILE,), "MW_GENERIC_RASTER": (E.PATH_GENERIC,)}.get(next(iter(env), ""), None)
    render_and_compare(angle_scenes(s0, carried), None, msaa, f"PutNext, {label}", path=want_path, views=(msaa == 8 and not env))


def test_carried_box_at_large_angles_off_the_tile_grid():
    """The same at 84 x 84 (the ragged tile kernels)."""
    s0, carried = putnext_carried()
    render_and_compare(angle_scenes(s0, carried), None, 8, "PutNext 84x84", size=(84, 84))


@pytest.mark.parametrize("env,msaa,label", [({}, 8, "mesh entity kernel"), ({"MW_K2Q": "0"}, 8, "mesh tiles"),
                                            ({"MW_GENERIC_RASTER": "1"}, 4, "generic kernel, 4 samples")])
def test_ball_and_key_meshes_at_large_angles(env, msaa, label, monkeypatch):
    """PickupObjects with domain randomisation: ball and key meshes at the angles, one of them carried in front of the
    camera, across the frame's lower border (the slow path's clipped triangles), the others where they stand."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s0 = first_scene("pickup_dr_s1")
    meshes = helpers.golden_meshes(s0)
    mesh_ents = [k for k in range(len(s0["ents_kind"])) if s0["ents_mesh"][k] >= 0 and not s0["ents_static"][k]]
    assert len(mesh_ents) >= 2, "the fixture holds fewer than two balls / keys"
    for carried in mesh_ents[:2]:
        render_and_compare(angle_scenes(s0, carried), meshes, msaa, f"PickupObjects-DR, {label}, carrying {carried}")


def test_maze_goal_box_at_large_angles():
    """The Maze's goal box through the big-scene kernels (mw_geom_big_kernel, mw_raster_big_kernel): every other env
    looks at it from 1.2 m, the others from where the agent stands in the fixture."""
    from miniworld_amd import engine as E
    s0 = first_scene("maze_s0")
    scenes = angle_scenes(s0, None)
    box = np.asarray(s0["ents_pos"][0], np.float64)
    for sc in scenes[::2]:
        a = float(sc["agent_dir"])
        sc["agent_pos"] = box - 1.2 * np.array([math.cos(a), 0.0, -math.sin(a)])
    render_and_compare(scenes, None, 8, "Maze goal box", path=(E.PATH_TILE,))


@pytest.mark.parametrize("domain_rand", [False, True])
def test_heading_the_device_accumulates_past_both_lines(domain_rand):
    """PutNext: a box placed in front of the agent is picked up, then 900 turns of 15 degrees take the agent's heading —
    and the carried box's, which copies it on every turn — from 0 to 235.6 rad, across 120 and 201.06 rad.  Frames on
    either side of each crossing, after a drop and after two steps back equal the oracle's render of the state the device
    holds, and the device's heading equals the host's f64 sum of the same turns, bit for bit.  (PutNext fixes
    max_episode_steps = 250, putnext.py:53: the step counter is reset through mw_set_state on the way.)"""
    import torch
    import pyoracle
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n = 4
    vec = MiniWorldVecEnv("MiniWorld-PutNext-v0", n, domain_rand=domain_rand, seed=11, autoreset=False)
    try:
        vec.reset()
        eng = vec.engine
        st = eng.get_state()
        t = vec.template
        cx, cz = (t.min_x + t.max_x) / 2, (t.min_z + t.max_z) / 2
        movable = [k for k in range(st["ent_kind"].shape[1]) if st["ent_kind"][0, k] != 0 and not st["ent_static"][0, k]]
        box = movable[0]
        pos = st["ent_pos"].copy()
        for j, k in enumerate(movable[1:]):                 # the other boxes along a wall, 2 m apart: nothing in the way
            pos[:, k] = [t.min_x + 1.0, 0.0, t.min_z + 1.0 + 2.0 * j]
        pos[:, box] = [cx + 0.7, 0.0, cz]                  # where the pickup's test circle finds it (miniworld.py:696-698)
        eng.set_state({"agent_pos": np.tile([cx, 0.0, cz], (n, 1)), "agent_dir": np.zeros(n), "ent_pos": pos,
                       "step_count": np.zeros(n, np.int32)})
        eng.set_step_params(np.tile([0.15, 0.0, 15.0], (n, 1)))
        act = lambda a: vec.step(torch.full((n,), a, dtype=torch.int32, device="cuda"))
        act(4)                                              # pickup
        st = eng.get_state()
        assert (st["carrying"] == box).all(), st["carrying"]

        def check(what, heading, carried):
            st = eng.get_state()
            obs = vec.obs.cpu().numpy()
            for i in range(n):
                assert st["agent_dir"][i] == heading, (what, i, st["agent_dir"][i], heading)
                assert st["ent_dir"][i, box] == heading, (what, i, st["ent_dir"][i, box], heading)
                assert st["carrying"][i] == (box if carried else -1), (what, i)
                want = pyoracle.render(helpers.scene_of_vec_env(vec, st, i))
                assert np.array_equal(obs[i], want["rgb"]), f"{what}, env {i}: {np.count_nonzero(obs[i] != want['rgb'])} RGB values differ"

        heading = 0.0
        checks = {458, 459, 767, 768, 769, 900}
        for turn in range(1, 901):
            if turn % 200 == 0:
                eng.set_state({"step_count": np.zeros(n, np.int32)})
            act(0)                                          # turn_left
            heading += 15.0 * (math.pi / 180)
            if turn in checks:
                check(f"turn {turn} ({heading:.2f} rad)", heading, True)
        assert 201.06 < heading < 240
        act(5)                                              # drop
        check("after the drop", heading, False)
        act(3)
        act(3)                                              # two steps back
        check("after two steps back", heading, False)
        eng.check()
    finally:
        vec.close()
