"""Frame reuse (mw_set_frame_reuse): a step leaves the rows of the envs whose frame did not change undrawn, and nothing a caller
sees differs from an engine that draws every env on every step.

Two batched envs take the same seeded random actions, A with reuse on and B with it off; observations, depth, rewards, flags and the
frame-clean bytes are compared bit for bit after every step.  That frames really are skipped — and only those the bytes name — is
shown with a sentinel: the test overwrites A's buffers while the engine still trusts them, and after the next step exactly the rows
of the clean envs still hold the sentinel.  Which (env, step) pairs are clean is checked against the CPU oracle's dynamics replayed
from the same seeds (helpers.EpisodeMirror): the move was `forward`, the pose did not change by a bit, the episode went on.

Families: Hallway, OneRoom with depth, PutNext and FourRooms (placement programs, boxes only) take the quad path and skip; the Maze
takes the tile kernel and skips; Sidewalk (the `program_rules` family), CollectHealth and PickupObjects hold mesh entities, so their
frames are drawn in full whatever the bytes say (CollectHealth's byte is never set)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

SENTINEL_U8, SENTINEL_F = 0xA5, -7.25
STEPS = 300


def _pair(env_id, n, seed, **kw):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    A = MiniWorldVecEnv(env_id, n, seed=seed, frame_reuse=True, **kw)
    B = MiniWorldVecEnv(env_id, n, seed=seed, frame_reuse=False, **kw)
    assert A.frame_reuse and A.engine.frame_reuse and not B.frame_reuse
    A.reset()
    B.reset()
    return A, B


def _actions(seed, steps, n, n_actions, p_fwd):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((steps, n)) < p_fwd, 2, rng.integers(0, n_actions, (steps, n)))


def _step_both(A, B, act, tag):
    """One step of both envs; everything a caller sees must agree.  Returns A's frame-clean bytes (== B's)."""
    import torch
    act = torch.as_tensor(act, dtype=torch.int32, device="cuda")
    oa, ra, ta, tra = (x.cpu().numpy() for x in A.step(act))
    ob, rb, tb, trb = (x.cpu().numpy() for x in B.step(act))
    bad = np.flatnonzero((oa != ob).reshape(len(oa), -1).any(axis=1))
    assert bad.size == 0, (tag, "obs rows differ", bad[:8])
    if A.depth is not None:
        assert np.array_equal(A.depth.cpu().numpy(), B.depth.cpu().numpy()), (tag, "depth")
    assert np.array_equal(ra, rb) and np.array_equal(ta, tb) and np.array_equal(tra, trb), (tag, "reward / flags")
    ca, cb = A.frame_clean().cpu().numpy(), B.frame_clean().cpu().numpy()
    assert np.array_equal(ca, cb) and set(np.unique(ca)) <= {0, 1}, (tag, "frame_clean bytes")
    return ca.astype(bool)


def _fill_sentinel(vec):
    vec.obs.fill_(SENTINEL_F if vec.obs.is_floating_point() else SENTINEL_U8)
    if vec.depth is not None:
        vec.depth.fill_(SENTINEL_F)


def _sentinel_rows(t):
    x = t.cpu().numpy().reshape(t.shape[0], -1)
    return np.all(x == (SENTINEL_F if np.issubdtype(x.dtype, np.floating) else SENTINEL_U8), axis=1)


def _skipped_rows_step(A, B, act, tag):
    """A step into buffers the test filled with a sentinel while the engine trusted them: the clean envs' rows keep the sentinel
    (they were not drawn), every other row is B's.  A's buffers are then drawn afresh.  Returns the clean mask."""
    import torch
    _fill_sentinel(A)
    act = torch.as_tensor(act, dtype=torch.int32, device="cuda")
    A.step(act)
    B.step(act)
    clean = A.frame_clean().cpu().numpy().astype(bool)
    assert np.array_equal(clean, B.frame_clean().cpu().numpy().astype(bool)), tag
    kept = _sentinel_rows(A.obs)
    assert np.array_equal(kept, clean), (tag, "rows left undrawn != clean envs", np.flatnonzero(kept != clean)[:8])
    oa, ob = A.obs.cpu().numpy(), B.obs.cpu().numpy()
    assert np.array_equal(oa[~clean], ob[~clean]), (tag, "drawn rows")
    if A.depth is not None:
        assert np.array_equal(_sentinel_rows(A.depth), clean), (tag, "depth rows left undrawn != clean envs")
        assert np.array_equal(A.depth.cpu().numpy()[~clean], B.depth.cpu().numpy()[~clean]), (tag, "drawn depth rows")
    # a whole frame: the buffers hold every env's current frame again (for an env whose step left a removal or a respawn behind its
    # frame that is the frame after it — such an env is not clean on its next step, which draws it)
    A.engine.render(A.obs, A.depth)
    return clean


def _run_pair(env_id, n, seed, n_actions, p_fwd=0.5, steps=STEPS, sentinel_every=37, path=None, **kw):
    """The lockstep run; returns (clean env-steps, env-steps, rows the sentinel steps found undrawn)."""
    from miniworld_amd import engine as eng
    A, B = _pair(env_id, n, seed, **kw)
    queue = _actions(seed, steps, n, n_actions, p_fwd)
    total = undrawn = 0
    for t in range(steps):
        if sentinel_every and t % sentinel_every == sentinel_every - 1:
            clean = _skipped_rows_step(A, B, queue[t], (env_id, t))
            undrawn += int(clean.sum())
        else:
            clean = _step_both(A, B, queue[t], (env_id, t))
        total += int(clean.sum())
    if path is not None:
        assert A.engine.raster_path() == getattr(eng, path) == B.engine.raster_path()
    for v in (A, B):
        v.engine.check()
        v.close()
    return total, steps * n, undrawn


# ------------------------------------------------------------------ which frames are clean: the oracle's dynamics

@pytest.mark.parametrize("env_id,cls_name,depth", [("MiniWorld-Hallway-v0", "Hallway", False), ("MiniWorld-OneRoom-v0", "OneRoom", True)])
def test_clean_steps_are_the_oracles_blocked_moves(env_id, cls_name, depth):
    """Without domain randomisation: frame_clean = 1 exactly on the (env, step) pairs where the oracle's dynamics say that the
    action was `forward`, the pose is bitwise the one before and the episode did not end (same-step auto-reset: an ended episode
    shows the next world).  K1 matches those dynamics to 1e-12 with identical flags, so the sets must be equal: a byte set where
    the oracle moved is a wrong frame, a byte missing where it did not is a frame drawn for nothing.  And the set is not empty."""
    from miniworld_amd import envs
    from miniworld_amd import engine as eng
    n, seed = 32, 4100
    A, B = _pair(env_id, n, seed, want_depth=depth)
    mirrors = [helpers.EpisodeMirror(getattr(envs, cls_name), seed + i, False, eng.TASK_GOTO) for i in range(n)]
    queue = _actions(seed, STEPS, n, 3, 0.4)
    n_clean = 0
    for t in range(STEPS):
        want = np.zeros(n, bool)
        for i, m in enumerate(mirrors):
            pos0, dir0 = m.state()[0:2]
            _, te, tr = m.step(int(queue[t, i]))
            pos1, dir1 = m.state()[0:2]
            same = pos0.tobytes() == pos1.tobytes() and np.float64(dir0).tobytes() == np.float64(dir1).tobytes()
            want[i] = queue[t, i] == 2 and same and not (te or tr)
        got = _step_both(A, B, queue[t], (env_id, t))
        assert np.array_equal(got, want), (env_id, t, "clean on the device only", np.flatnonzero(got & ~want)[:8],
                                           "in the oracle only", np.flatnonzero(want & ~got)[:8])
        n_clean += int(got.sum())
    share = n_clean / (STEPS * n)
    print(f"{env_id}: {n_clean} of {STEPS * n} env-steps clean ({100 * share:.1f} %)")
    assert n_clean > 0
    assert A.engine.raster_path() == eng.PATH_QUAD
    for v in (A, B):
        v.close()


# ------------------------------------------------------------------ every family: same outputs, rows really skipped

def test_hallway_same_step():
    clean, total, undrawn = _run_pair("MiniWorld-Hallway-v0", 48, 4200, 3, path="PATH_QUAD")
    assert clean > 0 and undrawn > 0


def test_oneroom_depth_next_step():
    clean, total, undrawn = _run_pair("MiniWorld-OneRoom-v0", 48, 4300, 3, want_depth=True, autoreset="next_step", path="PATH_QUAD")
    assert clean > 0 and undrawn > 0


def test_hallway_domain_rand_no_autoreset():
    """Per-step parameter draws move the random stream on a blocked move, not the frame; without auto-reset an ended episode stays."""
    clean, total, undrawn = _run_pair("MiniWorld-Hallway-v0", 32, 4400, 3, domain_rand=True, autoreset=False, steps=120, path="PATH_QUAD")
    assert clean > 0 and undrawn > 0


def test_putnext_boxes_picked_up_and_dropped():
    """Boxes are picked up, carried through turns a wall blocks, and dropped: a pickup or drop that finds nothing is clean, one that
    does something is not."""
    clean, total, undrawn = _run_pair("MiniWorld-PutNext-v0", 32, 4500, 8, p_fwd=0.3, path="PATH_QUAD")
    assert clean > 0 and undrawn > 0


def test_sidewalk_program_rules():
    """The rules that live in the placement program's tables (the forbidden street, the goal box).  The family's worlds hold mesh
    entities (the building, the cones), so its frames are drawn in full whatever the bytes say: the outputs must agree."""
    clean, total, undrawn = _run_pair("MiniWorld-Sidewalk-v0", 32, 4600, 3, sentinel_every=0)
    assert clean > 0


def test_four_rooms_program_family():
    """A placement-program family whose worlds hold boxes only: the quad path, frames skipped."""
    clean, total, undrawn = _run_pair("MiniWorld-FourRooms-v0", 32, 4650, 3, path="PATH_QUAD")
    assert clean > 0 and undrawn > 0


def test_collect_health_is_never_clean():
    """Its respawn kernel moves entities behind the step kernel's back: the byte is always 0, every frame is drawn."""
    clean, total, undrawn = _run_pair("MiniWorld-CollectHealth-v0", 24, 4700, 8, p_fwd=0.3)
    assert clean == 0 and undrawn == 0


def test_maze_tile_kernel():
    clean, total, undrawn = _run_pair("MiniWorld-MazeS3-v0", 24, 4800, 3, path="PATH_TILE")
    assert clean > 0 and undrawn > 0


def test_maze_tile_kernel_depth_next_step():
    clean, total, undrawn = _run_pair("MiniWorld-MazeS3-v0", 16, 4900, 3, want_depth=True, autoreset="next_step", steps=150, path="PATH_TILE")
    assert clean > 0 and undrawn > 0


def test_pickup_objects_sets_the_byte_but_draws_every_frame():
    """Frames with mesh entities are out of scope: the byte may be set, the frame is drawn in full — a buffer filled with a sentinel
    comes back without a row of it."""
    import torch
    from miniworld_amd import engine as eng
    A, B = _pair("MiniWorld-PickupObjects-v0", 24, 5000)
    queue = _actions(5000, STEPS, 24, 5, 0.4)
    n_clean = 0
    for t in range(STEPS):
        if t % 29 == 28:
            _fill_sentinel(A)
        clean = _step_both(A, B, queue[t], ("PickupObjects", t))       # (compares every row with B's: no sentinel survived)
        n_clean += int(clean.sum())
    assert n_clean > 0
    assert A.engine.raster_path() == eng.PATH_QUAD_MESH
    for v in (A, B):
        v.close()


def _short_episodes(monkeypatch, cls_name, steps):
    """Episodes of at most `steps` steps for a family whose class fixes max_episode_steps (the batched env and the mirrors read it
    from their instances)."""
    from miniworld_amd import envs
    base = getattr(envs, cls_name)

    class Short(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Short.__name__ = Short.__qualname__ = cls_name
    monkeypatch.setattr(envs, cls_name, Short)


def test_final_obs_steps_draw_everything_and_a_new_world_is_never_clean(monkeypatch):
    """Both passes of a step with final observations ignore the bytes.  The step kernel runs as a terminal step there and the
    install kernel replaces the finished envs' worlds behind it: an env truncated while it stands against a wall must not keep a
    set byte — its row now shows the next episode.  The bytes are the oracle's blocked moves of unfinished episodes, as without
    final observations, and 0 wherever terminated | truncated is set; the run has envs that ended on an unchanged frame."""
    from miniworld_amd import envs
    from miniworld_amd import engine as eng
    _short_episodes(monkeypatch, "Hallway", 40)
    n, seed, steps = 32, 5100, 240
    A, B = _pair("MiniWorld-Hallway-v0", n, seed, final_obs=True)
    mirrors = [helpers.EpisodeMirror(envs.Hallway, seed + i, False, eng.TASK_GOTO) for i in range(n)]
    queue = _actions(seed, steps, n, 3, 0.6)
    prev = A.obs.cpu().numpy().copy()
    ended_unchanged = n_clean = 0
    for t in range(steps):
        want = np.zeros(n, bool)
        for i, m in enumerate(mirrors):
            pos0, dir0 = m.state()[0:2]
            _, te, tr = m.step(int(queue[t, i]))
            pos1, dir1 = m.state()[0:2]
            want[i] = (queue[t, i] == 2 and not (te or tr) and pos0.tobytes() == pos1.tobytes()
                       and np.float64(dir0).tobytes() == np.float64(dir1).tobytes())
        if t % 7 == 6:
            _fill_sentinel(A)
        clean = _step_both(A, B, queue[t], ("final_obs", t))
        fin = A.final_obs.cpu().numpy()
        assert np.array_equal(fin, B.final_obs.cpu().numpy())
        done = (A.terminated | A.truncated).cpu().numpy().astype(bool)
        assert not (clean & done).any(), ("final_obs", t, "frame_clean set for an env that was given a new world", np.flatnonzero(clean & done)[:8])
        assert np.array_equal(clean, want), ("final_obs", t, np.flatnonzero(clean != want)[:8])
        ended_unchanged += int(sum(np.array_equal(fin[i], prev[i]) for i in np.flatnonzero(done)))
        n_clean += int(clean.sum())
        prev = A.obs.cpu().numpy().copy()
    assert n_clean > 0
    assert ended_unchanged > 0, "no episode ended on an unchanged frame: the check above met no such env"
    for v in (A, B):
        v.close()


# ------------------------------------------------------------------ when the buffer cannot be trusted

def _against_the_walls(A, B, n, tag, rounds=40):
    """Forward until a good part of the batch stands against a wall: the next forward step has clean envs."""
    for k in range(rounds):
        clean = _step_both(A, B, np.full(n, 2), (tag, "approach", k))
    assert clean.sum() >= 2, (tag, "too few blocked envs for the check to mean anything")


def _redrawn_after(A, B, n, tag, call):
    """`call(vec)` on both envs, with A's buffers full of sentinel: the next step has clean envs and still draws every row."""
    _step_both(A, B, np.full(n, 2), (tag, "before"))
    _fill_sentinel(A)
    call(A)
    call(B)
    clean = _step_both(A, B, np.full(n, 2), (tag, "after"))         # (every row equal to B's: all redrawn)
    return clean


def test_another_buffer_mid_run_redraws_everything():
    import torch
    n = 32
    A, B = _pair("MiniWorld-OneRoom-v0", n, 5200, want_depth=True, autoreset=False)
    _against_the_walls(A, B, n, "other buffer")
    other_obs, other_depth = torch.full_like(A.obs, SENTINEL_U8), torch.full_like(A.depth, SENTINEL_F)
    act = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    A.engine.step(act, other_obs, other_depth, A.reward, A.terminated, A.truncated)
    B.step(act)
    assert A.frame_clean().any()
    assert np.array_equal(other_obs.cpu().numpy(), B.obs.cpu().numpy()) and np.array_equal(other_depth.cpu().numpy(), B.depth.cpu().numpy())
    # back to the env's own tensors, which are one step behind: all of it again
    _fill_sentinel(A)
    clean = _step_both(A, B, np.full(n, 2), "back to the first buffer")
    assert clean.any()
    # the same obs with another depth pointer is another buffer too
    _step_both(A, B, np.full(n, 2), "settle")
    A.obs.fill_(SENTINEL_U8)
    A.engine.step(act, A.obs, other_depth, A.reward, A.terminated, A.truncated)
    B.step(act)
    assert A.frame_clean().any() and np.array_equal(A.obs.cpu().numpy(), B.obs.cpu().numpy())
    for v in (A, B):
        v.close()


def test_invalidating_entry_points_redraw_everything():
    """After each host-side writer of something a frame depends on, the next step draws every env, clean or not."""
    import torch
    from miniworld_amd import assets
    from miniworld_amd import engine as eng
    n = 32
    A, B = _pair("MiniWorld-OneRoom-v0", n, 5300, want_depth=True, autoreset=False)
    _against_the_walls(A, B, n, "invalidate")
    mask = np.zeros(n, np.uint8)
    mask[::5] = 1
    top = torch.zeros_like(A.obs)
    tex0 = sorted(A.tex_ids, key=A.tex_ids.get)[0]
    polys, segs = A.engine.get_geometry(0)
    calls = {
        "mw_reset (masked)": lambda v: v.engine.reset(mask, np.arange(n, dtype=np.uint64) + 77),
        "mw_set_state": lambda v: v.engine.set_state(v.engine.get_state()),
        "mw_set_geometry": lambda v: v.engine.set_geometry(-1, polys, segs.reshape(-1, 4)),
        "mw_upload_texture": lambda v: v.engine.upload_texture(0, assets.texture_rgb_bottom_up(tex0)),
        "mw_set_obs_layout": lambda v: v.engine.set_obs_layout(eng.OBS_HWC_U8),
        "mw_render_top": lambda v: v.engine.render_top(top, None, True),
        "mw_render_view": lambda v: v.engine.render_view(0, 64, 48, msaa=8),
        "mw_debug_set_mesh_frame_seq": lambda v: v.engine._check(v.engine.lib.mw_debug_set_mesh_frame_seq(v.engine.h, 3), "seq"),
        "mw_set_frame_reuse": lambda v: v.engine.set_frame_reuse(v.frame_reuse),
    }
    for name, call in calls.items():
        clean = _redrawn_after(A, B, n, name, call)
        assert clean.sum() >= 2, (name, "no clean env in the step after it: the check means nothing")
        # ... and the step after that one skips again
        skipped = _skipped_rows_step(A, B, np.full(n, 2), (name, "trusted again"))
        assert skipped.any(), name
    for v in (A, B):
        v.close()


def test_set_final_obs_and_gen_program_and_mesh_upload_invalidate():
    import torch
    from miniworld_amd.objmesh import ObjMesh
    n = 32
    A, B = _pair("MiniWorld-PutNext-v0", n, 5400)          # a placement-program family without mesh entities, same-step auto-reset
    _against_the_walls(A, B, n, "program family", rounds=60)
    def reinstall(v):       # the family's placement program, compiled again as MiniWorldVecEnv compiles it
        from miniworld_amd import genprog
        from miniworld_amd.scene import scene_from_env, upload_scene_meshes
        sc = scene_from_env(v.template)
        ents = [e for e in v.template.entities if e is not v.template.agent]
        mesh_map = upload_scene_meshes(v.engine, sc, v.mesh_ids, v.tex_ids)
        ops = genprog.family_ops(v.template, ents.index, v.template.rooms.index)
        v.engine.set_gen_program(*genprog.compile_program(v.template, sc, v.tex_ids, mesh_map, ops))
    clean = _redrawn_after(A, B, n, "mw_set_gen_program", reinstall)
    assert clean.any()
    clean = _redrawn_after(A, B, n, "mw_set_final_obs", lambda v: v.engine.set_final_obs(None))
    assert clean.any()
    assert _skipped_rows_step(A, B, np.full(n, 2), "trusted again").any()
    m = ObjMesh.get("ball_red")
    clean = _redrawn_after(A, B, n, "mw_upload_mesh", lambda v: v.engine.upload_mesh(0, m.verts, m.norms, m.texcs, m.colors))
    assert clean.any()
    for v in (A, B):
        v.close()
