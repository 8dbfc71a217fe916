"""The frame plan (mw_frame_plan_kernel) and the quad kernel that draws from it: in a plain step every env is left alone as clean,
copied from a slot of the frame cache or drawn, decided by a small kernel behind the geometry kernel, and the quad kernel's workgroups
take their env from the plan's lists — the first n_draw draw, the next n_copy copy, the rest leave.

For Hallway and OneRoom with depth at 8 samples, and Hallway at 4, batches of 1, 63, 64, 65 and 130 envs (whole and ragged plan
wavefronts; a launch whose workgroups split into drawing, copying and idle ones at every ratio) run one action script through six
engines at once — 1, 4 and 8 slots, frame reuse on and off.  After every step

 * the six engines hold the same state, and every env's frame (and depth map) in each of them equals the CPU oracle's render of that
   state bit for bit — rendered once per distinct state and shared;
 * mw_get_frame_source equals a host model of the rule, fed with the device's own states and clean bytes: clean wins where reuse
   applies, else the lowest slot whose key matches, else drawn into the round-robin victim; a hit changes nothing.

The script: L R L R L R L R (from the third step on every env is back in a state drawn two steps ago: every env copies, with at
least two slots), a drop with nothing in hand (no state changes: every env is clean with reuse on, and a hit on the frame drawn last
with reuse off — the only way to a copy with ONE slot, whose frame is always the previous state's), then a seeded mix of left, right
and forward.  Each of these must have occurred, or the test fails.  With one slot and reuse on no env can ever copy — a state equal
to the last drawn one is a clean env — so nothing is asked there; a step in which drawn, clean and copied envs sit side by side is
asked of the batches of 63 envs and more (reuse on, two slots and more; drawn and copied side by side otherwise)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

SLOTS, REUSE = (1, 4, 8), (True, False)
L, R, F, DROP = 0, 1, 2, 5
LR_STEPS, MIX_STEPS = 8, 10
_rendered = {}      # (family, samples, state bytes) -> the oracle's frame: shared by every engine, step and test of the module


def _script(n, seed):
    rng = np.random.default_rng(seed)
    rows = [np.full(n, (L, R)[t % 2]) for t in range(LR_STEPS)] + [np.full(n, DROP)]
    rows += [rng.choice([L, R, F, F], size=n) for _ in range(MIX_STEPS)]
    phase = ["lr"] * LR_STEPS + ["drop"] + ["mix"] * MIX_STEPS
    return np.stack(rows).astype(np.int32), phase


class _Model:
    """One env's cache on the host: the slots' (epoch, key), the slot the next drawn frame replaces, the epoch a new world advances."""

    def __init__(self, slots):
        self.keys, self.victim, self.epoch = [None] * slots, 0, 0

    def step(self, key, clean_skip, installed):
        if installed:
            self.epoch += 1
        if clean_skip:
            return 1
        k = (self.epoch, key)
        if k in self.keys:
            return 2 + self.keys.index(k)       # the lowest slot that holds it; nothing changes
        self.keys[self.victim] = k
        self.victim = (self.victim + 1) % len(self.keys)
        return 0


def _state_bytes(st, i):
    return b"".join(np.ascontiguousarray(st[f][i]).tobytes() for f in ("agent_pos", "agent_dir", "cam", "light", "ent_kind", "ent_pos", "ent_dir", "ent_geom"))


def _oracle(vec, family, samples, st, i):
    import pyoracle
    k = (family, samples, _state_bytes(st, i))
    if k not in _rendered:
        _rendered[k] = pyoracle.render(helpers.scene_of_vec_env(vec, st, i), nsamples=samples)
    return _rendered[k]


def _pose_keys(st):
    assert (st["carrying"] < 0).all()           # (nothing is ever picked up: the key is the agent's pose)
    pos, d = np.ascontiguousarray(st["agent_pos"], np.float64), np.ascontiguousarray(st["agent_dir"], np.float64)
    return [pos[i].tobytes() + d[i].tobytes() for i in range(len(d))]


def _check_step(tag, engines, family, samples, outs, models, reuse_applies):
    """Frames against the oracle, source bytes against the model, for every engine; returns the source bytes per engine."""
    import torch
    states = [v.engine.get_state() for v in engines]
    for st in states[1:]:
        for f in ("agent_pos", "agent_dir", "step_count", "ent_pos"):
            assert np.array_equal(st[f], states[0][f]), (tag, f, "the engines' states part")
    st = states[0]
    n = len(st["agent_dir"])
    want = [_oracle(engines[0], family, samples, st, i) for i in range(n)]
    rgb = np.stack([w["rgb"] for w in want])
    keys = _pose_keys(st)
    srcs = []
    for v, (obs, depth), ms, reuse in zip(engines, outs, models, reuse_applies):
        got = obs.cpu().numpy()
        bad = np.flatnonzero((got != rgb).reshape(n, -1).any(1))
        src = v.frame_source().cpu().numpy()
        assert bad.size == 0, (tag, "slots", v.frame_cache, "reuse", reuse, "frames differ from the oracle's: envs", bad[:8].tolist(), "source", src[bad[:8]].tolist())
        if depth is not None:
            z = np.stack([w["depth"] for w in want])
            bad = np.flatnonzero((depth.cpu().numpy() != z).reshape(n, -1).any(1))
            assert bad.size == 0, (tag, "slots", v.frame_cache, "reuse", reuse, "depth maps differ: envs", bad[:8].tolist(), "source", src[bad[:8]].tolist())
        clean = v.frame_clean().cpu().numpy().astype(bool)
        done = (v.terminated | v.truncated).cpu().numpy().astype(bool)
        model = np.array([ms[i].step(keys[i], bool(clean[i]) and reuse, bool(done[i])) for i in range(n)], np.uint8)
        bad = np.flatnonzero(src != model)
        assert bad.size == 0, (tag, "slots", v.frame_cache, "reuse", reuse, "envs", bad[:8].tolist(), "source", src[bad[:8]].tolist(), "model", model[bad[:8]].tolist())
        srcs.append(src)
    return srcs


CASES = [("MiniWorld-Hallway-v0", "Hallway", False, 8, n) for n in (1, 63, 64, 65, 130)] + \
        [("MiniWorld-OneRoom-v0", "OneRoom", True, 8, n) for n in (1, 63, 64, 65, 130)] + [("MiniWorld-Hallway-v0", "Hallway", False, 4, 65)]


@pytest.mark.parametrize("env_id,family,want_depth,samples,n", CASES, ids=[f"{c[1]}-{c[3]}x-{c[4]}" for c in CASES])
def test_frames_and_sources_follow_the_plan(env_id, family, want_depth, samples, n):
    import torch
    from miniworld_amd import engine as eng
    from miniworld_amd.vec_env import MiniWorldVecEnv
    combos = [(s, r) for s in SLOTS for r in REUSE]
    engines = [MiniWorldVecEnv(env_id, n, seed=9000 + n, frame_cache=s, frame_reuse=r, want_depth=want_depth, msaa=samples) for s, r in combos]
    for v, (s, r) in zip(engines, combos):
        assert v.frame_cache == s and v.frame_reuse == r
        v.reset()
    models = [[_Model(s) for _ in range(n)] for s, _ in combos]
    script, phase = _script(n, 77 + n)
    all_copy, all_clean, all_drawn, mixed = set(), set(), set(), set()
    for t in range(len(script)):
        act = torch.as_tensor(script[t], dtype=torch.int32, device="cuda")
        for v, (_, r) in zip(engines, combos):
            if not r:       # (reuse off: the engine promises nothing about what the buffers hold, and must write every row)
                v.obs.fill_(0xAA)
                if v.depth is not None:
                    v.depth.fill_(-1.0)
            v.step(act)
        srcs = _check_step((family, samples, n, "step", t, phase[t]), engines, family, samples, [(v.obs, v.depth) for v in engines], models,
                           [r for _, r in combos])
        for c, src in zip(combos, srcs):
            if (src >= 2).all():
                all_copy.add((c, phase[t]))
            if (src == 1).all():
                all_clean.add((c, phase[t]))
            if (src == 0).all() and t == 0:
                all_drawn.add(c)
            if phase[t] == "mix" and (src == 0).any() and (src >= 2).any() and ((src == 1).any() or not c[1]):
                mixed.add(c)
    for v in engines:
        assert v.engine.raster_path() == eng.PATH_QUAD
        v.engine.check()
        v.close()
    for c in combos:
        s, r = c
        assert c in all_drawn, (c, "the first step after the reset did not draw every env")
        if s >= 2:
            assert (c, "lr") in all_copy, (c, "no step of the L R L R phase in which every env copied")
        if r:
            assert (c, "drop") in all_clean, (c, "the drop with nothing in hand did not leave every env alone")
        else:
            assert (c, "drop") in all_copy, (c, "with reuse off every env of the drop step is a hit on the frame drawn last")
            assert not any(k[0] == c for k in all_clean), (c, "an env was left alone though reuse is off")
        if n >= 63 and s >= 2:
            assert c in mixed, (c, "no step of the random mix in which drawn" + (", clean" if r else "") + " and copied envs share the launch")


@pytest.mark.parametrize("offset", [0, 4, 1])
def test_two_caller_buffers_at_every_alignment(offset):
    """The caller alternates between two buffer sets `offset` bytes off a 16-byte boundary: frame reuse cannot apply (no env is left
    alone), the cache still hits, and the copy takes its 16-, 4- or 1-byte store path; drawn and copied rows alike equal the oracle's."""
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, family = 65, "OneRoom"
    v = MiniWorldVecEnv("MiniWorld-OneRoom-v0", n, seed=9000 + n, frame_cache=4, want_depth=True)
    v.reset()
    sets = []
    for _ in range(2):
        raw = torch.zeros(v.obs.numel() + 16, dtype=torch.uint8, device="cuda")
        rawz = torch.zeros(v.depth.numel() + 4, dtype=torch.float32, device="cuda")
        obs = raw[offset:offset + v.obs.numel()].view(v.obs.shape)
        depth = rawz[(offset + 3) // 4:(offset + 3) // 4 + v.depth.numel()].view(v.depth.shape)
        assert obs.data_ptr() % 16 == offset and depth.data_ptr() % 16 == 4 * ((offset + 3) // 4)
        sets.append((obs, depth))
    models = [[_Model(4) for _ in range(n)]]
    script, phase = _script(n, 77 + n)
    copied = drawn = 0
    for t in range(len(script)):
        obs, depth = sets[t % 2]
        obs.fill_(0xAA)         # (the L R steps would otherwise find the frame of two steps ago, the one they must write, already there)
        depth.fill_(-1.0)
        v.engine.step(torch.as_tensor(script[t], dtype=torch.int32, device="cuda"), obs, depth, v.reward, v.terminated, v.truncated)
        src = _check_step((family, "offset", offset, "step", t, phase[t]), [v], family, 8, [(obs, depth)], models, [False])[0]
        assert not (src == 1).any(), (t, "an env was left alone in a buffer that does not hold its frame")
        copied += int((src >= 2).sum())
        drawn += int((src == 0).sum())
        if phase[t] == "drop":
            assert (src >= 2).all(), "every env of the drop step is a hit on the frame drawn last"
    assert copied > n * 4 and drawn > n * 4, (copied, drawn)
    v.engine.check()
    v.close()
