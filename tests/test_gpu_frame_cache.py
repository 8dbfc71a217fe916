"""The frame cache (mw_set_frame_cache): an env that is back in a state whose frame the engine drew a few steps ago gets a copy of that
frame instead of a new drawing, and nothing a caller sees differs from an engine that draws every env on every step.

1. Differential: three batched envs take the same seeded actions, the cache off, with two and with four slots; observations, depth,
   rewards and flags are compared bit for bit after every step.  67 envs (a ragged last dense wavefront), episodes of at most 30 steps
   so that worlds are installed and episodes time out all along the run.
2. Hits happen, and the replacement is round-robin over the drawn frames: scripted turns on Hallway against a host model of the
   cache that is fed with the device's own states (mw_get_state) — no arithmetic is assumed on the host.
3. Invalidation: every host-side writer of something a frame depends on drops the cached frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, EPISODE = 67, 200, 30


def _short_episodes(monkeypatch, cls_name, steps=EPISODE):
    """Episodes of at most `steps` steps for a family whose class fixes max_episode_steps."""
    from miniworld_amd import envs
    base = getattr(envs, cls_name)

    class Short(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.max_episode_steps = steps
    Short.__name__ = Short.__qualname__ = cls_name
    monkeypatch.setattr(envs, cls_name, Short)


def _make(env_id, n, seed, slots, **kw):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    v = MiniWorldVecEnv(env_id, n, seed=seed, frame_cache=slots, **kw)
    assert v.frame_cache == slots == v.engine.frame_cache
    v.reset()
    return v


def _actions(seed, steps, n, n_actions, p_turn):
    """Seeded actions with many reversed turns in them: turns with probability p_turn, else uniform over the family's actions."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((steps, n)) < p_turn, rng.integers(0, 2, (steps, n)), rng.integers(0, n_actions, (steps, n)))


class _Out:
    """The output tensors of one env for steps that do not go to its own: `alt` alternates between two sets, `offset` places them
    that many bytes off a 16-byte boundary."""

    def __init__(self, v, alt, offset):
        import torch
        self.v, self.k = v, 0
        self.sets = []
        for _ in range(2 if alt else 1):
            if not alt and not offset:
                self.sets.append((v.obs, v.depth))
                continue
            raw = torch.zeros(v.obs.numel() + 16, dtype=torch.uint8, device="cuda")
            obs = raw[offset:offset + v.obs.numel()].view(v.obs.shape)
            depth = None
            if v.depth is not None:
                rawz = torch.zeros(v.depth.numel() + 4, dtype=torch.float32, device="cuda")
                depth = rawz[(offset + 3) // 4:(offset + 3) // 4 + v.depth.numel()].view(v.depth.shape)
            assert obs.data_ptr() % 16 == offset % 16
            self.sets.append((obs, depth))

    def step(self, act, repeat):
        v = self.v
        obs, depth = self.sets[self.k % len(self.sets)]
        self.k += 1
        if obs is v.obs:
            v.step(act, repeat=repeat)
        elif repeat == 1:
            v.engine.step(act, obs, depth, v.reward, v.terminated, v.truncated)
        else:
            v.engine.step_repeat(act, repeat, obs, depth, v.reward, v.terminated, v.truncated)
        return obs, depth


def _differential(monkeypatch, env_id, cls_name, n_actions, seed, *, repeat=1, alt=False, offset=0, p_turn=0.6, expect_hits=True, **kw):
    import torch
    from miniworld_amd import engine as eng
    _short_episodes(monkeypatch, cls_name)
    vs = [_make(env_id, N, seed, slots, **kw) for slots in (0, 2, 4)]
    outs = [_Out(v, alt, offset) for v in vs]
    queue = _actions(seed, STEPS, N, n_actions, p_turn)
    hits, clean_hits, ends = [0, 0, 0], 0, 0
    for t in range(STEPS):
        act = torch.as_tensor(queue[t], dtype=torch.int32, device="cuda")
        res = [o.step(act, repeat) for o in outs]
        ref_obs, ref_depth = res[0]
        for k in (1, 2):
            obs, depth = res[k]
            assert torch.equal(obs, ref_obs), (env_id, t, vs[k].frame_cache, "obs rows differ",
                                              torch.nonzero((obs != ref_obs).reshape(N, -1).any(1)).flatten()[:8].tolist())
            if ref_depth is not None:
                assert torch.equal(depth, ref_depth), (env_id, t, vs[k].frame_cache, "depth")
            assert torch.equal(vs[k].reward, vs[0].reward) and torch.equal(vs[k].terminated, vs[0].terminated) and \
                torch.equal(vs[k].truncated, vs[0].truncated), (env_id, t, "reward / flags")
            assert torch.equal(vs[k].frame_clean(), vs[0].frame_clean()), (env_id, t, "frame_clean")
        ends += int((vs[0].terminated | vs[0].truncated).sum())
        for k, v in enumerate(vs):
            src = v.frame_source()
            assert int(src.max()) <= 1 + v.frame_cache, (env_id, t, "source byte names a slot the cache does not have")
            hits[k] += int((src >= 2).sum())
            if k == 2 and alt:
                # other buffers than the last step's: frame reuse skips nothing, and a clean env is an ordinary hit
                assert not bool((src == 1).any()), (env_id, t, "an env was left undrawn in a buffer that does not hold its frame")
                clean_hits += int(((src >= 2) & (v.frame_clean() == 1)).sum())
    assert ends > N, "too few episodes ended for installs and time-outs to have been exercised"
    assert hits[0] == 0
    if expect_hits:
        assert vs[2].engine.raster_path() == eng.PATH_QUAD
        assert hits[2] >= hits[1] > 0, hits
        if alt:
            assert clean_hits > 0, "no clean env among the hits: the case shows nothing about other buffers"
    else:
        assert hits == [0, 0, 0], hits
    for v in vs:
        v.engine.check()
        v.close()
    return hits


def test_hallway(monkeypatch):
    hits = _differential(monkeypatch, "MiniWorld-Hallway-v0", "Hallway", 3, 6100)
    assert hits[2] > 0.15 * N * STEPS, ("a turn-heavy policy revisits more than this", hits)


def test_oneroom_with_depth(monkeypatch):
    _differential(monkeypatch, "MiniWorld-OneRoom-v0", "OneRoom", 3, 6200, want_depth=True)


def test_a_frame_size_off_the_grid_takes_no_cache(monkeypatch):
    """81 x 61 is not drawn by the quad kernel: the setting is held, nothing is cached, nothing differs."""
    _differential(monkeypatch, "MiniWorld-Hallway-v0", "Hallway", 3, 6300, obs_width=81, obs_height=61, expect_hits=False)


def test_another_frame_size_on_the_grid(monkeypatch):
    _differential(monkeypatch, "MiniWorld-OneRoom-v0", "OneRoom", 3, 6350, want_depth=True, obs_width=64, obs_height=44)


def test_boxes_picked_up_and_dropped(monkeypatch):
    """PutNext: boxes without meshes; pickup and drop are in the action mix, so carried slots change and dropped boxes stay where
    they were put — poses that return do not bring the old frame back."""
    _differential(monkeypatch, "MiniWorld-PutNext-v0", "PutNext", 8, 6400, p_turn=0.35)


def test_next_step_autoreset(monkeypatch):
    _differential(monkeypatch, "MiniWorld-Hallway-v0", "Hallway", 3, 6500, autoreset="next_step")


def test_action_repeat(monkeypatch):
    _differential(monkeypatch, "MiniWorld-PutNext-v0", "PutNext", 8, 6600, repeat=3, p_turn=0.35)
    _differential(monkeypatch, "MiniWorld-Hallway-v0", "Hallway", 3, 6650, repeat=3, autoreset="next_step")


@pytest.mark.parametrize("reuse", [True, False])
def test_with_and_without_frame_reuse(monkeypatch, reuse):
    _differential(monkeypatch, "MiniWorld-OneRoom-v0", "OneRoom", 3, 6700, want_depth=True, frame_reuse=reuse, p_turn=0.3)


@pytest.mark.parametrize("offset", [0, 4, 1])
def test_the_caller_alternates_between_two_buffers(monkeypatch, offset):
    """... which frame reuse cannot follow and the cache need not: it still hits, clean envs included.  The buffers also sit off a
    16-byte boundary (by 4 bytes, by 1): the copy's other store widths."""
    _differential(monkeypatch, "MiniWorld-OneRoom-v0", "OneRoom", 3, 6800 + offset, want_depth=True, alt=True, offset=offset, p_turn=0.3)


# ------------------------------------------------------------------ hits and replacement against a model of the cache

class _Model:
    """What the engine's cache of one env holds, from the device's own states: slots of (epoch, key bytes), the slot the next drawn
    frame replaces, the epoch that an installed world advances."""

    def __init__(self, slots):
        self.slots, self.keys, self.victim, self.epoch = slots, [None] * slots, 0, 0

    def step(self, key, clean_skip, installed):
        """The source byte this step's frame must report."""
        if installed:
            self.epoch += 1
        if clean_skip:
            return 1
        k = (self.epoch, key)
        if k in self.keys:
            return 2 + self.keys.index(k)
        self.keys[self.victim] = k
        self.victim = (self.victim + 1) % self.slots
        return 0


def _keys(v):
    st = v.engine.get_state()
    assert (st["carrying"] < 0).all()          # (Hallway: nothing to carry, the key is the agent's pose)
    pos, d = np.ascontiguousarray(st["agent_pos"], np.float64), np.ascontiguousarray(st["agent_dir"], np.float64)
    return [pos[i].tobytes() + d[i].tobytes() for i in range(len(d))]


@pytest.mark.parametrize("script", ["LR", "LLRR"])
def test_hits_and_round_robin_replacement(monkeypatch, script):
    import torch
    _short_episodes(monkeypatch, "Hallway", 22)        # (time-outs inside the run: an installed world parts the frames)
    n, steps = 24, 48
    vs = {slots: _make("MiniWorld-Hallway-v0", n, 7100, slots) for slots in (2, 4)}
    models = {slots: [_Model(slots) for _ in range(n)] for slots in vs}
    src = {slots: np.zeros((steps, n), np.uint8) for slots in vs}
    keys = []
    done_at = np.zeros((steps, n), bool)
    for t in range(steps):
        a = {"L": 0, "R": 1}[script[t % len(script)]]
        act = torch.full((n,), a, dtype=torch.int32, device="cuda")
        for slots, v in vs.items():
            v.step(act)
            src[slots][t] = v.frame_source().cpu().numpy()
            done = (v.terminated | v.truncated).cpu().numpy().astype(bool)
            clean = v.frame_clean().cpu().numpy().astype(bool)
            k = _keys(v)
            want = np.array([models[slots][i].step(k[i], bool(clean[i]) and v.frame_reuse, bool(done[i])) for i in range(n)], np.uint8)
            bad = np.flatnonzero(src[slots][t] != want)
            assert bad.size == 0, (script, slots, t, "envs", bad[:8], "source", src[slots][t][bad[:8]], "model", want[bad[:8]])
        keys.append(k)
        done_at[t] = done
    assert done_at.any(), "no episode ended inside the run"
    for slots in vs:
        assert (src[slots] >= 2).any(), (script, slots, "no hit at all")
    if script == "LLRR":
        # the second R of a cycle returns to the state two R's and two L's ago.  Between that frame and this one three others were
        # drawn: with two slots it is gone, with four it is still there.
        seen = 0
        for t in range(7, steps, 4):
            for i in range(n):
                if keys[t][i] == keys[t - 4][i] and not done_at[t - 4 + 1:t + 1, i].any() and src[4][t - 4][i] == 0 \
                        and all(keys[t - j][i] != keys[t][i] for j in (1, 2, 3)):
                    seen += 1
                    assert src[2][t][i] == 0, (t, i, "two slots cannot hold a frame drawn four distinct frames ago")
                    assert src[4][t][i] >= 2, (t, i, "four slots hold it")
        assert seen > 0, "no env returned to the bits of the state four steps earlier: the check met nothing"
    for v in vs.values():
        v.engine.check()
        v.close()


# ------------------------------------------------------------------ invalidation

def _turn(vs, a, tag):
    """One turn step of the cached env and the uncached one; their frames must agree.  Returns the cached env's source bytes."""
    import torch
    A, B = vs
    act = torch.full((A.num_envs,), a, dtype=torch.int32, device="cuda")
    A.step(act)
    B.step(act)
    bad = torch.nonzero((A.obs != B.obs).reshape(A.num_envs, -1).any(1)).flatten()
    assert bad.numel() == 0, (tag, "the cached env shows other frames than the uncached one, envs", bad[:8].tolist())
    if A.depth is not None:
        assert torch.equal(A.depth, B.depth), (tag, "depth")
    return A.frame_source().cpu().numpy()


def _move_the_box(v):
    st = v.engine.get_state()
    st["ent_pos"] = st["ent_pos"].copy()
    st["ent_pos"][:, 0, 0] -= 1.5               # the goal box, along the hallway towards the agent
    v.engine.set_state(st)


def _other_texture(v):
    for tex_id in sorted(v.tex_ids.values()):
        rgb = np.zeros((32, 32, 3), np.uint8)
        rgb[::2, :, 0] = 255
        v.engine.upload_texture(tex_id, rgb)


def _layout_there_and_back(v):
    from miniworld_amd import engine as eng
    v.engine.set_obs_layout(eng.OBS_CWH_U8)
    v.engine.set_obs_layout(eng.OBS_HWC_U8)


INVALIDATORS = {
    "mw_set_state": _move_the_box,
    "mw_upload_texture": _other_texture,
    "mw_reset": lambda v: v.reset(seed=991),
    "mw_set_obs_layout": _layout_there_and_back,
}


@pytest.mark.parametrize("name", list(INVALIDATORS) + ["mw_snapshot_load"])
def test_host_side_writers_drop_the_cache(name):
    """L, R, L brings every env into a state whose key is cached (the third step hits); then R, the call, and L again: the pose is
    that of a cached frame, what the frame shows is not.  The frames must be the uncached env's."""
    import torch
    n = 24
    A = _make("MiniWorld-Hallway-v0", n, 7300, 4, want_depth=True, autoreset=False)
    B = _make("MiniWorld-Hallway-v0", n, 7300, 0, want_depth=True, autoreset=False)
    vs = (A, B)
    _turn(vs, 0, (name, "L"))
    _turn(vs, 1, (name, "R"))
    src = _turn(vs, 0, (name, "L again"))
    assert (src >= 2).sum() > n // 2, (name, "the run-up does not hit: the case shows nothing", src)
    _turn(vs, 1, (name, "R again"))
    if name == "mw_snapshot_load":
        # the states of a run whose box stands elsewhere, loaded over this one: same agent poses, same epochs, other frames
        C = _make("MiniWorld-Hallway-v0", n, 7300, 0, want_depth=True, autoreset=False)
        _move_the_box(C)
        for a in (0, 1, 0, 1):
            C.step(torch.full((n,), a, dtype=torch.int32, device="cuda"))
        snap = C.save_state()
        for v in vs:
            v.load_state(snap)
        C.close()
    else:
        for v in vs:
            INVALIDATORS[name](v)
            v.engine.render(v.obs, v.depth)
    src = _turn(vs, 0, (name, "L after the call"))
    assert not (src >= 2).any(), (name, "a frame from before the call was handed out", src)
    _turn(vs, 1, (name, "R after the call"))
    src = _turn(vs, 0, (name, "the cache fills again"))
    assert (src >= 2).sum() > n // 2, (name, src)
    for v in vs:
        v.engine.check()
        v.close()
