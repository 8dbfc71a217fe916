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

This module is the class's core — the constructor's steps, the buffers, reset, step, rollout, the state views and the infos — and the
import path of everything around it: the configuration (env_config.py), the snapshots and level banks (snapshots.py), the "levels" and
"seeds" restarts (restarts.py) and the world queries (queries.py) join the class as mixins; the argument rules are _args.py's.
"""
from __future__ import annotations

import numpy as np

from . import engine as eng
from . import envs as _envs
from ._args import integer, seeds_u64
from .env_config import _INFO_KIND, _KIND, AUTORESET_MODES, EnvConfig, _ball_key_meshes, _entity_slots, build_config   # noqa: F401 (re-exported)
from .queries import DepthMap, DepthWindow, EgoWindow, LabelFrame, NavField, ObjectMap, ObjectWindow, SeenMap, WorldQueries     # noqa: F401
from .restarts import Restarts
from .scene import polys_array, scene_from_env, state_arrays, upload_scene_meshes
from .snapshots import EnvSnapshot, Snapshots           # noqa: F401


class MiniWorldVecEnv(Snapshots, Restarts, WorldQueries):
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
        self.frame_stack = None if frame_stack is None else integer("MiniWorldVecEnv", "frame_stack", frame_stack, 2, eng.MAX_STACK)
        if stack_pad not in ("reset", "zero"):
            raise ValueError(f"stack_pad must be 'reset' or 'zero', not {stack_pad!r}")
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
        self._ego_bufs = {}             # ego_update()'s samples per (size, dtype), made on first use
        self._fork_buf = None           # fork()'s scratch records, made on first use
        self._fork_frames = None        # ... and its scratch frame records (fork(src, frames=True))
        self._done = self._done_b = self._done_i = None     # the finished envs of a step as uint8 / bool / int64 ("levels", "seeds")

    def _set_frame_options(self, frame_reuse, frame_cache, final_obs):
        """frame reuse, the frame cache and the frame stack, in that order"""
        torch, n = self.torch, self.num_envs
        self.frame_reuse = self.engine.set_frame_reuse(frame_reuse)
        self.frame_cache = self.engine.set_frame_cache(integer("MiniWorldVecEnv", "frame_cache", frame_cache, 0, eng.MAX_FRAME_CACHE))
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

    def _device_mask(self, mask, where, name="mask"):
        """nav_field / raycast / seen_update: None, or a uint8 / bool [N] tensor already on the device; a bool is viewed as bytes (one
        byte per element, 0 / 1: no conversion kernel)"""
        torch = self.torch
        if mask is None:
            return None
        if (not torch.is_tensor(mask) or tuple(mask.shape) != (self.num_envs,) or mask.dtype not in (torch.uint8, torch.bool)
                or mask.device != self.engine.device):
            raise ValueError(f"{where}: {name} is a uint8 or bool tensor [{self.num_envs}] on {self.engine.device}")
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
            seeds_u64("reset", [self._next_seed, self._next_seed + 2 * self.num_envs - 1], below=2 ** 63)       # (episode_seed and next_seed are int64)
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
            seeds = torch.from_numpy(seeds_u64("reset_where", seeds).view(np.int64))
        elif seeds.device.type == "cpu" and seeds.dtype == torch.int64:
            seeds_u64("reset_where", seeds.numpy(), below=2 ** 63)
        mask, seeds = self._copied_mask(mask), seeds.to(device=dev, dtype=torch.int64).contiguous()
        self.engine.reset_where(mask, seeds)
        if self.episode_seed is not None:
            torch.where(mask != 0, seeds, self.episode_seed, out=self.episode_seed)
        return self._redraw()

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
                slot = integer("rollout", "trace_ent", slot, 0, self.engine.cfg.max_ents - 1)
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
                                        trace=bufs, ent_slot=slot if "ent_pos" in names else 0)
        if self.autoreset_mode == "levels":
            self._finished_to_levels(frames=render)
        elif self.next_seed is not None:
            self._advance_seeds()
        return obs, self.reward, self.terminated, self.truncated

    def _info_buffer(self, name):
        """what get_info / get_final_info fill for this env's `info` key, made on first use: health int32[N], goal_pos float64[N, 3]"""
        if self._info_kind == "health":
            return self._buffer(name, (self.num_envs,), self.torch.int32)
        return self._buffer(name, (self.num_envs, 3), self.torch.float64)

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
