"""Gymnasium VectorEnv-style adapter over MiniWorldVecEnv.

    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", num_envs=4096)
    obs, infos = envs.reset(seed=0)
    obs, rewards, terminations, truncations, infos = envs.step(actions)

follows gymnasium.vector.VectorEnv's calling convention (num_envs, single_* / batched spaces,
reset -> (obs, infos), step -> 5-tuple, autoreset mode "same-step" by default: the observation returned with
a finished episode is the first one of the next episode; or "next-step", below; `levels=` chooses the worlds, further below).  Observations, rewards and flags stay
torch tensors on the engine's GPU by default (`to_numpy=True` copies them to the host like a
classic VectorEnv); actions may be a torch tensor, a numpy array or a list.

**A same-step consumer gets `final_obs` on request: `final_obs=True`.**  Gymnasium's SAME_STEP mode promises the finished
episode's last observation under info["final_obs"].  By default the engine does not draw it (the step's only frame is the next
episode's first one — the reference leaves resets to the caller and renders once per step, miniworld.py:670-730), and no
"final_obs" key is emitted.  With `final_obs=True` every step draws the finished envs' terminal frames as well (a second, small
frame of those envs in the same step, on the device) and info carries "final_obs" (the batch's observation array: the rows
masked by info["_final_obs"] hold the terminal frames, the others are undefined; a copy, valid after the next step) and
"_final_obs" (bool[N], the envs whose episode ended with this step).  SB3's `terminal_observation` and gymnasium 0.29's
`final_observation` are the same rows.  Always there: info["_final_info"] (bool[N], for every env family, also those
without info keys) and — for the families that have info keys (CollectHealth's health, TMaze / YMaze's goal_pos) —
info["final_info"], the finished episodes' own values.  The arrays under final_info are copies: they stay valid after the
next step.

**`autoreset_mode="next-step"` gives the terminal observation** (gymnasium's AutoresetMode.NEXT_STEP, its default for vector envs
since 1.0; `metadata["autoreset_mode"]` of the instance says so): the step that ends an episode returns that episode's last frame,
reward, flags and info (CollectHealth's final health, TMaze / YMaze's goal_pos of that episode) — no "final_obs" / "final_info"
keys are needed and none are emitted —, and the env's next step ignores its action and returns the next episode's first frame
with reward 0 and both flags False.  `self.vec.reset_pending()` marks the envs whose next step is such a reset step.  Still one
frame per env and step, drawn in the same kernels; the worlds follow the reference's "step; if done: reset()" stream order.

**The observation returned with `to_numpy=False` is the engine's own device tensor: treat it as read-only between steps.**  A
step does not redraw an env whose state did not change (a move into a wall, a pickup that finds nothing): its rows already hold
that frame (`MiniWorldVecEnv(frame_reuse=True)`, the default).  A wrapper that normalises or augments observations IN PLACE would
find its own writes again in the rows of such envs — copy first (`obs.clone()`, `obs.float()`), or pass `frame_reuse=False`, which
draws every env on every step.  `to_numpy=True` hands out host copies and is not affected.  Results are bit for bit the same
either way; `self.vec.frame_clean()` tells a consumer which rows did not change.

**`frame_cache`: on for exploration, off for a policy that never turns back.**  The engine keeps every env's last `frame_cache` (default 4)
distinct drawn frames on the device and copies one instead of drawing when the env is back in the state it shows — a third of the steps
of a near-uniform policy, +15 % env-steps/s on Hallway.  A policy that never returns to a state gains nothing and pays one more store
of every frame: -3.7 % with always-turn-left (against `frame_cache=0`; the step with the cache on has since become faster under that
policy, 13.36 -> 13.48 M with the frame plan, profiles/r20, and 13.41 -> 14.21 M with its draw list ordered by cost, profiles/r22).  For
such a consumer:

    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", num_envs=4096, frame_cache=0)

Results are bit for bit the same either way; it costs 59 MB of device memory per slot at 4096 envs of 80x60 (78 MB more with depth).

**`levels=`: a finite set of worlds.**  `levels=seeds` (an integer sequence or tensor) builds a bank with one level per seed — level l is
the reference's `env.reset(seed=seeds[l])` with its first observation —, `levels=snapshot` takes one (MiniWorldVecEnv.make_levels /
save_state(frames=True)).  Finished envs then restart from a record of the bank in the same step, on the device (MiniWorldVecEnv's
autoreset="levels"): the adapter advertises same-step auto-reset, info["level"] (int32[N]) is the level each env played in the step that
just ended, and `self.vec.next_level` (int32[N] on the device) is the caller's to write between steps — a training set and a held-out
set are two banks, a level-replay sampler writes its choices there.  final_obs is not available in this mode.

**`reset_seeds=`: worlds by seed, unbounded.**  `reset_seeds=True` (MiniWorldVecEnv's autoreset="seeds") makes the same-step auto-reset
start the reference's `env.reset(seed=next_seed[i])` for a finished env i, generated on the device: `self.vec.next_seed` (int64[N] on the
device) is the caller's to write between steps, `info["seed"]` (int64[N]) is the seed each env played in the step that just ended.
`reset_seeds=tensor` (or a sequence) also writes it as the first `next_seed`.  Left alone, env i walks seed + i, seed + N + i, ...
Eight bytes per level instead of a record; composes with final_obs.
"""
from __future__ import annotations

import numpy as np

from .gymshim import AUTORESET_NEXT_STEP, AUTORESET_SAME_STEP, VectorEnvBase, batch_action_space, spaces
from .vec_env import MiniWorldVecEnv


class MiniWorldVectorEnv(VectorEnvBase):
    """A gymnasium.vector.VectorEnv when gymnasium is importable (a plain class with the same surface otherwise)."""
    metadata = {"autoreset_mode": AUTORESET_SAME_STEP, "render_modes": ["rgb_array"]}

    def __init__(self, env_id: str, num_envs: int, to_numpy: bool = False, autoreset_mode="same-step", final_obs: bool = False,
                 frame_reuse: bool = True, frame_cache: int = 4, action_repeat: int = 1, frame_stack: int | None = None, stack_pad: str = "reset",
                 levels=None, level_generator=None, reset_seeds=None, info_state=None, seen_map=None, ego_map=None, depth_map=None, label_frame=None, object_map=None,
                 **kwargs):
        """autoreset_mode: "same-step" (the class's metadata) or "next-step" (module docstring); gymnasium's AutoresetMode values
        are accepted too.  final_obs (same-step only): info["final_obs"] / info["_final_obs"] (module docstring).  frame_reuse:
        False draws every env on every step, for consumers that write into the returned observation tensor (module docstring).
        frame_cache: slots per env of the engine's cache of drawn frames (MiniWorldVecEnv's frame_cache; 0 turns it off).
        action_repeat > 1: every step() holds the action for up to that many env steps (MiniWorldVecEnv.step's `repeat`) and
        info["substeps"] (int32[N]) tells how many each env took.
        frame_stack=K, stack_pad: observations (and the observation spaces) become the stacks of the last K frames, oldest first
        (MiniWorldVecEnv's frame_stack: Gymnasium's FrameStackObservation / SB3's VecFrameStack on the device) — the engine's
        view, read-only until the next step, or a host copy with to_numpy; with final_obs, info["final_obs"] holds the final
        stacks (the old stack with the terminal frame appended).
        levels: seeds or an EnvSnapshot with frame records — finished envs restart from that bank (module docstring); same-step only,
        without final_obs.  level_generator: the torch.Generator of the uniform draws of next_level.
        reset_seeds: True, or the first next_seed (int64[N] tensor / sequence) — finished envs restart from `vec.next_seed` (module
        docstring); same-step only, excludes levels= and autoreset=.
        info_state: names of state fields (MiniWorldVecEnv.state: "agent_pos", "agent_dir", "carrying", "ent_pos", ...) — every
        step() and reset() adds them to info as arrays over the batch, filled by one gather kernel behind the step; None (the
        default) adds nothing.  The rows show the state the device holds, as the other info keys do: for an env whose episode ended
        with the step that is its next episode's first state under the same-step auto-reset, the terminal state under next-step.
        Copies: they stay valid after the next step.
        seen_map: a dict of MiniWorldVecEnv.seen_map()'s arguments (an empty one for its defaults) — every step() marks what each agent
        sees from its new pose in an explored-area map on the device (`self.seen`, a SeenMap) and adds info["seen_new"] (int32[N], the
        cells that became seen with this step: a coverage reward) and info["seen_count"] (int32[N], the cells seen so far in the
        episode); the map of an env whose episode ended restarts with the first pose of its next one (under next-step with the reset
        step), and reset() restarts every map.  None (the default) adds nothing and calls nothing.
        ego_map: a dict of MiniWorldVecEnv.ego_window()'s arguments (an empty one for its defaults) — reset() and every step() fill an
        egocentric map window around each agent's new pose on the device (`self.ego`, an EgoWindow; one kernel) and add info["ego_map"],
        uint8[N, P, S, S]: its planes, a cheap symbolic observation.  For an env whose episode ended with the step the window shows what the
        device holds: its next episode's world under the same-step auto-reset.  A copy: it stays valid after the next step.  None (the
        default) adds nothing and calls nothing.
        depth_map: a dict of MiniWorldVecEnv.depth_window()'s arguments (an empty one for its defaults) — the env draws depth maps
        (want_depth is switched on; want_depth=False beside it is refused), reset() and every step() project the new depth map into an
        egocentric window on the device (`self.depth_win`, a DepthWindow; one kernel) and add info["depth_map"], uint8[N, 2, S, S]: the
        floor and obstacle points per cell, the map a policy without simulator state may have — laid out like ego_map's planes, which
        are its labels.  A copy: it stays valid after the next step.  None (the default) adds nothing and calls nothing.
        label_frame: a dict of MiniWorldVecEnv.label_frame()'s arguments (an empty one for its defaults) — reset() and every step() cast
        what each pixel of the new observation shows on the device (`self.label`, a LabelFrame; one kernel) and add info["label"]: that
        LabelFrame itself, whose tensors the next step rewrites (clone what must outlive it).  For an env whose episode ended with the
        step the labels show what the device holds, like the observation under the same-step auto-reset.  None (the default) adds
        nothing and calls nothing.
        object_map: a dict of MiniWorldVecEnv.object_window()'s arguments (an empty one for its defaults) — needs label_frame= with `code`
        (ValueError otherwise); reset() and every step() project the new labels into an egocentric window on the device behind the label
        update (`self.object_win`, an ObjectWindow; one kernel; the label frame's own depth where it has one, else the env's, for which
        want_depth is switched on) and add info["object_map"], uint8[N, S, S]: 1 + the entity slot sensed in each cell, 0 for none —
        laid out like ego_map's entity plane, which is its label.  A copy: it stays valid after the next step.  None (the default)
        adds nothing and calls nothing."""
        if object_map is not None:
            if not isinstance(object_map, dict):
                raise ValueError(f"object_map: need a dict of MiniWorldVecEnv.object_window()'s arguments or None, not {object_map!r}")
            if not isinstance(label_frame, dict) or label_frame.get("code", True) is not True:
                raise ValueError("object_map= projects the label frame's codes: it needs label_frame= (a dict) with code=True")
            if label_frame.get("depth", False) is not True:
                if kwargs.get("want_depth", True) is not True:
                    raise ValueError("object_map= needs a depth map: label_frame=dict(depth=True), or the env's own (it excludes want_depth=False)")
                kwargs["want_depth"] = True
        if label_frame is not None and not isinstance(label_frame, dict):
            raise ValueError(f"label_frame: need a dict of MiniWorldVecEnv.label_frame()'s arguments or None, not {label_frame!r}")
        if depth_map is not None:
            if not isinstance(depth_map, dict):
                raise ValueError(f"depth_map: need a dict of MiniWorldVecEnv.depth_window()'s arguments or None, not {depth_map!r}")
            if kwargs.get("want_depth", True) is not True:
                raise ValueError("depth_map= needs the env's depth maps: it excludes want_depth=False")
            kwargs["want_depth"] = True
        if seen_map is not None and not isinstance(seen_map, dict):
            raise ValueError(f"seen_map: need a dict of MiniWorldVecEnv.seen_map()'s arguments or None, not {seen_map!r}")
        if ego_map is not None and (not isinstance(ego_map, dict) or ego_map.get("planes", True) in ((), [])):
            raise ValueError(f"ego_map: need a dict of MiniWorldVecEnv.ego_window()'s arguments with at least one plane, or None, not {ego_map!r}")
        if not isinstance(action_repeat, (int, np.integer)) or not 1 <= action_repeat <= 256:
            raise ValueError(f"action_repeat must be an integer in 1 .. 256, not {action_repeat!r}")
        self.action_repeat = int(action_repeat)
        kwargs["frame_reuse"] = frame_reuse
        kwargs["frame_cache"] = frame_cache
        if frame_stack is not None:
            kwargs["frame_stack"], kwargs["stack_pad"] = frame_stack, stack_pad
        mode = str(getattr(autoreset_mode, "name", autoreset_mode)).lower().replace("_", "-")     # (an AutoresetMode: its name)
        if mode not in ("same-step", "next-step"):
            raise ValueError(f"autoreset_mode must be 'same-step' or 'next-step', not {autoreset_mode!r}")
        if mode == "next-step":
            if kwargs.get("autoreset", True) is not True:
                raise ValueError("autoreset_mode='next-step' and autoreset= exclude each other")
            kwargs["autoreset"] = "next_step"
            self.metadata = dict(type(self).metadata, autoreset_mode=AUTORESET_NEXT_STEP)
        if final_obs and mode != "same-step":
            raise ValueError("final_obs=True needs autoreset_mode='same-step' (next-step returns the terminal frame itself)")
        if final_obs:
            kwargs["final_obs"] = True
        if levels is not None:
            if mode != "same-step" or final_obs or kwargs.get("autoreset", True) is not True:
                raise ValueError("levels= is the same-step auto-reset from a bank: it excludes autoreset_mode='next-step', autoreset= and final_obs=True")
            kwargs["autoreset"] = "levels"
        seeded = reset_seeds is not None and reset_seeds is not False
        if seeded:
            if mode != "same-step" or levels is not None or kwargs.get("autoreset", True) is not True:
                raise ValueError("reset_seeds= is the seeded same-step auto-reset: it excludes autoreset_mode='next-step', autoreset= and levels=")
            kwargs["autoreset"] = "seeds"
        from .engine import STATE_FIELDS
        self.info_state = None if info_state is None else tuple(info_state)
        if self.info_state is not None and (isinstance(info_state, str) or not self.info_state or any(k not in STATE_FIELDS for k in self.info_state)):
            raise ValueError(f"info_state: need a sequence of state field names out of {sorted(STATE_FIELDS)}, not {info_state!r}")
        self.vec = MiniWorldVecEnv(env_id, num_envs, **kwargs)
        self._first_next_seed = None
        if seeded and reset_seeds is not True:
            first = np.asarray(reset_seeds.detach().cpu().numpy() if hasattr(reset_seeds, "detach") else reset_seeds)
            if first.shape != (num_envs,) or first.dtype.kind not in "iu" or (first < 0).any():
                raise ValueError(f"reset_seeds: need True or {num_envs} non-negative integers")
            self._first_next_seed = self.vec.torch.from_numpy(first.astype(np.int64)).to(self.vec.engine.device)
            self.vec.next_seed.copy_(self._first_next_seed)
        self._played_seed = None
        self.seen = None if seen_map is None else self.vec.seen_map(**seen_map)
        self._seen_clear = None         # next-step: the envs whose next step is their reset step
        self.ego = None if ego_map is None else self.vec.ego_window(**ego_map)
        self.depth_win = None if depth_map is None else self.vec.depth_window(**depth_map)
        self.label = None if label_frame is None else self.vec.label_frame(**label_frame)
        self.object_win = None if object_map is None else self.vec.object_window(**object_map)
        if levels is not None:
            from .vec_env import EnvSnapshot
            self.vec.set_levels(levels if isinstance(levels, EnvSnapshot) else self.vec.make_levels(levels), level_generator)
        self.num_envs = num_envs
        self.to_numpy = to_numpy
        shape, dtype = tuple(self.vec.obs.shape[1:]), {"grey": np.float64}.get(self.vec.obs_layout, np.uint8)
        if self.vec.frame_stack:
            shape = (self.vec.frame_stack,) + shape
        self.single_observation_space = spaces.Box(0, 255, shape, dtype=dtype)
        self.observation_space = spaces.Box(0, 255, (num_envs,) + shape, dtype=dtype)
        self.single_action_space = spaces.Discrete(self.vec.n_actions)
        self.action_space = batch_action_space(self.single_action_space, num_envs)
        self.render_mode = "rgb_array"
        self.closed = False

    def _out(self, t):
        return t.cpu().numpy() if self.to_numpy else t

    def _obs(self, obs):
        return self.vec.stack if self.vec.frame_stack else obs

    def _infos(self):
        """gymnasium's batched info convention: one array per key (health / goal_pos: MiniWorldVecEnv.infos)."""
        return {k: self._out(v) for k, v in self.vec.infos().items()}

    def _state_info(self, info):
        """info_state: the named fields of the state the device holds, one state() call; copies (state()'s tensors are reused)"""
        if self.info_state is not None:
            for k, v in self.vec.state(self.info_state).items():
                info[k] = self._out(v) if self.to_numpy else v.clone()
        return info

    def _seen_info(self, info, done, all_new):
        """seen_map: one seen_update() behind the step or reset; copies of the map's counters (they are rewritten by the next step)"""
        if self.seen is not None:
            torch = self.vec.torch
            if all_new:
                clear = torch.ones(self.num_envs, dtype=torch.uint8, device=self.vec.engine.device)
            elif self.vec.autoreset_mode == "next_step":
                clear = self._seen_clear
            else:
                clear = done.to(torch.uint8) if self.vec.autoreset_mode != "off" else None
            self._seen_clear = None if all_new else done.to(torch.uint8)
            self.vec.seen_update(self.seen, clear=clear)
            info["seen_new"] = self._out(self.seen.new) if self.to_numpy else self.seen.new.clone()
            info["seen_count"] = self._out(self.seen.count) if self.to_numpy else self.seen.count.clone()
        return info

    def _ego_info(self, info):
        """ego_map: one ego_update() behind the step or reset; a copy of the window's planes (they are rewritten by the next step)"""
        if self.ego is not None:
            planes = self.vec.ego_update(self.ego)
            info["ego_map"] = self._out(planes) if self.to_numpy else planes.clone()
        return info

    def _depth_info(self, info):
        """depth_map: one depth_update() behind the step or reset; a copy of the window's planes (they are rewritten by the next step)"""
        if self.depth_win is not None:
            planes = self.vec.depth_update(self.depth_win)
            info["depth_map"] = self._out(planes) if self.to_numpy else planes.clone()
        return info

    def _label_info(self, info):
        """label_frame: one label_update() behind the step or reset; the LabelFrame itself (its tensors are rewritten by the next step)"""
        if self.label is not None:
            self.vec.label_update(self.label)
            info["label"] = self.label
        return info

    def _object_info(self, info):
        """object_map: one object_update() behind the label update; a copy of the window's plane (it is rewritten by the next step)"""
        if self.object_win is not None:
            plane = self.vec.object_update(self.object_win, self.label)
            info["object_map"] = self._out(plane) if self.to_numpy else plane.clone()
        return info

    def reset(self, *, seed: int | None = None, options: dict | None = None):
        """Env i is seeded with seed + i (gymnasium's convention for an integer seed); with levels= every env starts a level of the
        bank and the seed is not used."""
        obs = self.vec.reset(seed)
        if self._first_next_seed is not None:       # (reset() lays out seed + N + i; the caller's first choices stand)
            self.vec.next_seed.copy_(self._first_next_seed)
        return self._out(self._obs(obs)), self._state_info(self._object_info(self._label_info(self._depth_info(self._ego_info(self._seen_info({}, None, True))))))

    def step(self, actions):
        torch = self.vec.torch
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions), device=self.vec.engine.device)
        actions = actions.to(device=self.vec.engine.device, dtype=torch.int32)
        if self.vec.autoreset_mode == "seeds":      # the seed each env plays in this step (the step moves episode_seed on)
            if self._played_seed is None:
                self._played_seed = torch.zeros_like(self.vec.episode_seed)
            self._played_seed.copy_(self.vec.episode_seed)
        obs, rew, term, trunc = self.vec.step(actions, self.action_repeat)
        info = self._infos()
        if self.action_repeat > 1:
            info["substeps"] = self._out(self.vec.substeps) if self.to_numpy else self.vec.substeps.clone()
        if self.vec.autoreset_mode in ("same_step", "levels", "seeds"):
            # gymnasium's same-step convention: "_final_info" masks the envs whose episode ended with this step (every family); the
            # finished episodes' own info under "final_info" where the family has info keys — clones, the engine's buffers are
            # rewritten by the next step.  ("final_obs" with final_obs=True: see the module's docstring.)
            done = self._out((term | trunc).bool())
            info["_final_info"] = done
            if self.vec.final_obs is not None:
                final = self.vec.final_stack if self.vec.frame_stack else self.vec.final_obs
                info["final_obs"] = self._out(final) if self.to_numpy else final.clone()
                info["_final_obs"] = done
            if info.keys() - {"_final_info"}:
                final = {k: (self._out(v) if self.to_numpy else v.clone()) for k, v in self.vec.final_infos().items()}
                final.update({"_" + k: done for k in list(final)})
                info["final_info"] = final
        if self.vec.autoreset_mode == "levels":
            info["level"] = self._out(self.vec.played_level) if self.to_numpy else self.vec.played_level.clone()
        if self.vec.autoreset_mode == "seeds":
            info["seed"] = self._out(self._played_seed) if self.to_numpy else self._played_seed.clone()
        self._seen_info(info, term | trunc, False)
        self._ego_info(info)
        self._depth_info(info)
        self._label_info(info)
        self._object_info(info)
        self._state_info(info)
        return self._out(self._obs(obs)), self._out(rew), self._out(term.bool()), self._out(trunc.bool()), info

    def render(self):
        """Tuple-free batched render: the map view of every env (uint8[N, H, W, 3])."""
        return self._out(self.vec.render_top_view())

    def get_visible_ents(self):
        return self._out(self.vec.get_visible_ents())

    def close(self):
        if not self.closed:
            self.vec.close()
            self.closed = True
