"""The ordered frame plan: mw_frame_plan_kernel files every draw entry under the cost class of its env's display-list length, and the
quad kernel's workgroups take the entries from the highest class down (mw_frame_plan.h: mw_plan_cost_class, mw_plan_slot) — the
frames that take longest start first.  No result may depend on that order.

Hallway at 8 and at 4 samples and OneRoom with depth at 8, batches of 1, 65 and 130 envs (one ragged plan wavefront, two, three:
the smallest shapes at which a wrong base or prefix of the class counts shows), frame reuse and a 4-slot frame cache on.  Eight steps
of per-env random left / right / forward / drop: a drop with nothing in hand and a blocked move leave an env clean, a turn that undoes
the last one is a hit on the frame drawn two steps ago, everything else is drawn — all three side by side in one launch.  After every
step

 * every env's frame (and depth map) equals the CPU oracle's render of the device's state bit for bit;
 * mw_get_frame_source equals the host model of the rule (clean wins, else the lowest matching slot, else drawn);
 * the plan block (mw_get_frame_plan) holds as draw entries exactly the envs whose source byte says drawn, each once, with the
   round-robin victim slot of the model, and as copy entries exactly the hits with their slot; the head's counts agree;
 * along the draw list, in the order the workgroups take it, the cost class — recomputed here from the lengths the accessor
   returns — never increases.

At 130 envs at least one step must populate two classes or more, and at 65 and 130 envs drawn, clean and copied envs must have shared
a step, or the test fails.  One case runs a second engine of the same seed that is reset in the middle of the script (its cached
frames dropped, every env drawn in the step behind it; the order has no state of its own that a reset could leave stale — the class
comes from the frame's own display list): its frames and its plan blocks are held to the oracle and the source bytes in the same way."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

L, R, F, DROP = 0, 1, 2, 5
STEPS, SLOTS, CLASSES = 8, 4, 8
_rendered = {}      # (family, samples, state bytes) -> the oracle's frame, shared by every step and case of the module


def _script(n, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.choice([L, R, F, F, DROP], size=n) for _ in range(STEPS)]
    # (the step behind a reset turns every env: no env is clean while the caller's buffers do not yet hold the last step's frames)
    rows[0], rows[STEPS // 2] = np.full(n, L), np.full(n, R)
    return np.stack(rows).astype(np.int32)


class _Model:
    """One env's cache on the host: the slots' (epoch, key), the slot the next drawn frame replaces, the epoch a new world advances."""

    def __init__(self, slots):
        self.keys, self.victim, self.epoch = [None] * slots, 0, 0

    def step(self, key, clean_skip, installed):
        """(source byte, the slot a drawn frame goes to or a copied one comes from)"""
        if installed:
            self.epoch += 1
        if clean_skip:
            return 1, 0
        k = (self.epoch, key)
        if k in self.keys:
            return 2 + self.keys.index(k), self.keys.index(k)
        v = self.victim
        self.keys[v] = k
        self.victim = (v + 1) % len(self.keys)
        return 0, v


def _state_bytes(st, i):
    return b"".join(np.ascontiguousarray(st[f][i]).tobytes() for f in ("agent_pos", "agent_dir", "cam", "light", "ent_kind", "ent_pos", "ent_dir", "ent_geom"))


def _oracle(vec, family, samples, st, i):
    import pyoracle
    k = (family, samples, _state_bytes(st, i))
    if k not in _rendered:
        _rendered[k] = pyoracle.render(helpers.scene_of_vec_env(vec, st, i), nsamples=samples)
    return _rendered[k]


def _check_frames(tag, v, family, samples, st):
    n = len(st["agent_dir"])
    want = [_oracle(v, family, samples, st, i) for i in range(n)]
    src = v.frame_source().cpu().numpy()
    bad = np.flatnonzero((v.obs.cpu().numpy() != np.stack([w["rgb"] for w in want])).reshape(n, -1).any(1))
    assert bad.size == 0, (tag, "frames differ from the oracle's: envs", bad[:8].tolist(), "source", src[bad[:8]].tolist())
    if v.depth is not None:
        bad = np.flatnonzero((v.depth.cpu().numpy() != np.stack([w["depth"] for w in want])).reshape(n, -1).any(1))
        assert bad.size == 0, (tag, "depth maps differ: envs", bad[:8].tolist(), "source", src[bad[:8]].tolist())
    return src


def _check_plan(tag, v, src, slot_of=None, ordered=True, slots=SLOTS):
    """The block against the source bytes (and the model's slots); returns the classes along the draw list.  v: a MiniWorldVecEnv or
    an Engine.  ordered=False (tests/test_gpu_launch_shapes.py: 65536 envs and more): one draw list, no classes; returns its envs."""
    p =getattr(v, "engine", v).get_frame_plan()
    if not ordered:
        assert p["classes"] == 0 and p["class_counts"] == [], (tag, "a batch this large gets one unordered draw list", p["classes"])
        assert not p["block"][[32, 33, 64, 65]].any(), (tag, "class counts in the head of an unordered plan")
        return _check_lists(tag, p, src, slot_of, slots)
    assert p["classes"] == CLASSES, (tag, "a batch this small gets an ordered plan")
    denv = _check_lists(tag, p, src, slot_of, slots)
    assert p["n_draw"] == sum(p["class_counts"]), (tag, p["n_draw"], p["class_counts"])
    cls = np.minimum(CLASSES - 1, np.maximum(p["lengths"], 0) // 4)[denv]
    assert (np.diff(cls) <= 0).all(), (tag, "the classes along the draw list increase somewhere", cls.tolist()[:64])
    assert [int((cls == c).sum()) for c in range(CLASSES)] == p["class_counts"], (tag, "the head's class counts", p["class_counts"])
    return cls


def _check_lists(tag, p, src, slot_of, slots):
    """the draw and copy entries of a plan block against the source bytes; returns the envs along the draw list"""
    denv, dslot = (p["draw"] & 0xFFFFFF).astype(np.int64), (p["draw"] >> 24).astype(np.int64)
    cenv, cslot = (p["copy"] & 0xFFFFFF).astype(np.int64), (p["copy"] >> 24).astype(np.int64)
    assert p["n_draw"] == denv.size == int((src == 0).sum()), (tag, p["n_draw"], p["class_counts"], int((src == 0).sum()))
    assert p["n_copy"] == cenv.size == int((src >= 2).sum()), (tag, p["n_copy"], int((src >= 2).sum()))
    assert np.array_equal(np.sort(denv), np.flatnonzero(src == 0)), (tag, "the draw entries are not the drawn envs, each once")
    assert np.array_equal(np.sort(cenv), np.flatnonzero(src >= 2)), (tag, "the copy entries are not the hits, each once")
    assert (cslot == src[cenv].astype(np.int64) - 2).all(), (tag, "a copy entry names another slot than the source byte")
    if slot_of is not None:
        assert (dslot == slot_of[denv]).all(), (tag, "a draw entry names another victim slot than the rule's", denv[dslot != slot_of[denv]][:8].tolist())
    else:
        assert (dslot < slots).all()
    return denv


CASES = [("MiniWorld-Hallway-v0", "Hallway", False, 8, n) for n in (1, 65, 130)] + [("MiniWorld-Hallway-v0", "Hallway", False, 4, n) for n in (1, 65, 130)] + \
        [("MiniWorld-OneRoom-v0", "OneRoom", True, 8, n) for n in (1, 65, 130)]


@pytest.mark.parametrize("env_id,family,want_depth,samples,n", CASES, ids=[f"{c[1]}-{c[3]}x-{c[4]}" for c in CASES])
def test_frames_sources_and_the_plan_block_under_the_ordered_plan(env_id, family, want_depth, samples, n):
    import torch
    from miniworld_amd import engine as eng
    from miniworld_amd.vec_env import MiniWorldVecEnv
    v = MiniWorldVecEnv(env_id, n, seed=2200 + n, frame_cache=SLOTS, frame_reuse=True, want_depth=want_depth, msaa=samples)
    assert v.frame_cache == SLOTS and v.frame_reuse
    v.reset()
    models = [_Model(SLOTS) for _ in range(n)]
    script = _script(n, 22 + n)
    most_classes, mixed = 0, False
    for t in range(STEPS):
        v.step(torch.as_tensor(script[t], dtype=torch.int32, device="cuda"))
        tag = (family, samples, n, "step", t)
        st = v.engine.get_state()
        src = _check_frames(tag, v, family, samples, st)
        assert (st["carrying"] < 0).all()           # (nothing is ever picked up: the key is the agent's pose)
        pos, d = np.ascontiguousarray(st["agent_pos"], np.float64), np.ascontiguousarray(st["agent_dir"], np.float64)
        clean = v.frame_clean().cpu().numpy().astype(bool)
        done = (v.terminated | v.truncated).cpu().numpy().astype(bool)
        verdicts = [models[i].step(pos[i].tobytes() + d[i].tobytes(), bool(clean[i]), bool(done[i])) for i in range(n)]
        model = np.array([s for s, _ in verdicts], np.uint8)
        bad = np.flatnonzero(src != model)
        assert bad.size == 0, (tag, "envs", bad[:8].tolist(), "source", src[bad[:8]].tolist(), "model", model[bad[:8]].tolist())
        cls = _check_plan(tag, v, src, np.array([s for _, s in verdicts], np.int64))
        most_classes = max(most_classes, len(set(cls.tolist())))
        mixed |= bool((src == 0).any() and (src == 1).any() and (src >= 2).any())
    assert v.engine.raster_path() == eng.PATH_QUAD
    v.engine.check()
    v.close()
    if n >= 65:
        assert mixed, "no step in which drawn, clean and copied envs share the launch"
    if n == 130:
        assert most_classes >= 2, "no step whose draw list holds two cost classes: the order was never put to the test"


def test_an_engine_reset_in_the_middle_of_the_script_draws_the_same_frames():
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    n, family = 65, "Hallway"
    twins = [MiniWorldVecEnv("MiniWorld-Hallway-v0", n, seed=2200 + n, frame_cache=SLOTS, frame_reuse=True) for _ in range(2)]
    for v in twins:
        v.reset()
    script = _script(n, 22 + n)
    for t in range(STEPS):
        if t == STEPS // 2:
            twins[1].reset()            # every cached frame of this engine is dropped; from here on its states are its own
        for k, v in enumerate(twins):
            v.step(torch.as_tensor(script[t], dtype=torch.int32, device="cuda"))
            tag = (family, "twin", k, "step", t)
            src = _check_frames(tag, v, family, 8, v.engine.get_state())
            _check_plan(tag, v, src)
        if t == STEPS // 2:
            assert (twins[1].frame_source().cpu().numpy() == 0).all(), "the step behind a reset draws every env"
    for v in twins:
        v.engine.check()
        v.close()
