"""A CPU model of the public stepping API (MiniWorldVecEnv), with nothing of the engine in it: no torch, no HIP, no engine code.

`ModelEnv` is one environment: the host world generator (`cls(host_only=True, ...)`, seed-exact with the reference's reset(),
tests/test_host_logic_cpu.py), the C oracle's dynamics (pyoracle.Dynamics, pinned on the reference's trajectories), the three per-step
domain-randomisation draws from the env's own numpy stream in the reference's order (miniworld.py:677-680) and pyoracle.render for the
frames.  `ModelVec` is a batch of them behind the method names of MiniWorldVecEnv, written from the contracts of include/mwengine.h,
the MiniWorldVecEnv docstrings and DESIGN §5 — what a call MEANS, in the plainest Python that says it: lists of frames for the stacks,
field-by-field copies for the snapshot records, a loop over the envs for every call.  tests/test_engine_model_cpu.py checks it here;
tests/test_gpu_api_fuzz.py drives the engine and this model with the same op sequences.

Out of scope: CollectHealth (its respawn draws are pinned through the env API only), navigation fields and ray casts (read-only, each
has a numpy reference of its own), autoreset="levels" (its loads are the masked loads modelled here), rollout(render=False)."""
import copy
import ctypes as C
import itertools

import numpy as np

_world_ids = itertools.count(1)


class ModelEnv:
    """One environment.  `sc` is the neutral scene of the episode's world as reset() built it and is never written; the live state
    is `dyn` (agent and entities; `dyn.render_ents`: the entities as the last step's frame shows them, before PickupObjects removes
    what was picked up, pickupobjects.py:86-88); the stream is `h.np_random`."""

    def __init__(self, cls, seed, domain_rand, task, **env_kwargs):
        self.h = cls(host_only=True, domain_rand=domain_rand, **env_kwargs)
        self.dr, self.task = domain_rand, task
        self.episodes = 0
        self.reset(seed)

    @classmethod
    def from_scene(cls, scene, task, max_episode_steps, goal_ent=0, goal_ent2=-1, agent_radius=0.4):
        """An env over a given neutral scene (a golden fixture's s0): no generator and no stream, so no reset(); substep() then needs
        its three per-step parameters."""
        m = cls.__new__(cls)
        m.h, m.dr, m.task, m.episodes = None, False, task, 0
        m._install(scene, dict(max_episode_steps=int(max_episode_steps), goal_ent=int(goal_ent), goal_ent2=int(goal_ent2),
                               num_objs=len(scene["ents_kind"]), max_forward_step=float(scene["max_forward_step"]),
                               agent_radius=float(agent_radius)))
        return m

    # ------------------------------------------------------------------ worlds
    def reset(self, seed=None):
        """MiniWorldEnv.reset(seed=seed): a new stream from the seed, or (None) the next world of the stream the env is on."""
        if seed is None:
            self.h.reset()
        else:
            self.h.reset(seed=int(seed))
        self._new_episode()

    def _new_episode(self):
        from miniworld_amd.scene import scene_from_env
        h = self.h
        sc = scene_from_env(h)
        ents = [e for e in h.entities if e is not h.agent]
        # PutNext's rule (putnext.py:74-78) is about two of the boxes; every other task rule is about slot 0 or about none
        g0, g1 = (ents.index(h.red_box), ents.index(h.yellow_box)) if hasattr(h, "red_box") else (0, -1)
        self._install(sc, dict(max_episode_steps=int(min(float(h.max_episode_steps), 2 ** 30)), goal_ent=g0, goal_ent2=g1,
                               num_objs=len(sc["ents_kind"]), max_forward_step=float(h.max_forward_step),
                               agent_radius=float(h.agent.radius)))

    def _install(self, sc, dyn_kw):
        import pyoracle
        self.sc, self.dyn_kw = sc, dyn_kw
        self.dyn = pyoracle.Dynamics(sc, self.task, **dyn_kw)
        self.fresh = True
        self.episodes += 1
        self.world_id = next(_world_ids)

    # ------------------------------------------------------------------ steps
    def substep(self, action, params=None):
        """One MiniWorldEnv.step(action) and the env's rule, without any auto-reset: (reward, terminated, truncated).  params: the
        (forward_step, forward_drift, turn_step) to use instead of the draws."""
        if params is None:
            rand = self.h.np_random if self.dr else None
            params = [self.h.params.sample(rand, k) for k in ("forward_step", "forward_drift", "turn_step")]
        r, te, tr = self.dyn.step(int(action), *params)
        self.fresh = False
        return r, te, tr

    @property
    def E(self):
        return len(self.sc["ents_kind"])

    def state(self):
        """(agent_pos, agent_dir, carrying, step_count, alive[E], ent_pos[E,3], ent_dir[E]) after the last step."""
        E = self.E
        ag, ents = self.dyn.ag, self.dyn.ents
        return (np.array(ag.pos[:]), float(ag.dir), int(ag.carrying), int(ag.step_count),
                np.array([bool(ents[k].alive) for k in range(E)]),
                np.array([ents[k].pos[:] for k in range(E)]).reshape(E, 3), np.array([ents[k].dir for k in range(E)]))

    def _scene_with(self, ents):
        sc = dict(self.sc)
        E = self.E
        ag = self.dyn.ag
        sc["agent_pos"], sc["agent_dir"] = np.array(ag.pos[:]), np.float64(ag.dir)
        sc["ents_pos"] = np.array([ents[k].pos[:] for k in range(E)]).reshape(E, 3)
        sc["ents_dir"] = np.array([ents[k].dir for k in range(E)])
        sc["ents_kind"] = np.where([bool(ents[k].alive) for k in range(E)], sc["ents_kind"], 0).astype(np.int32)
        return sc

    def frame_scene(self):
        """The scene the observation returned by the last step shows: a fresh episode's initial world, or the state
        at render time — rendering happens before PickupObjects removes what was picked up (pickupobjects.py:86-88)."""
        return dict(self.sc) if self.fresh else self._scene_with(self.dyn.render_ents)

    def scene_now(self):
        """The scene a frame drawn NOW shows (mw_render between steps): the live state, a removed object gone."""
        return dict(self.sc) if self.fresh else self._scene_with(self.dyn.ents)

    def key(self, ents=None):
        """Everything a frame of this env depends on, as bytes: the world and the poses."""
        ents = self.dyn.ents if ents is None else ents
        ag = self.dyn.ag
        return (self.world_id, bytes(ag.pos), np.float64(ag.dir).tobytes(), C.string_at(ents, C.sizeof(ents)))

    def frame_key(self):
        return self.key(self.dyn.ents if self.fresh else self.dyn.render_ents)

    def meshes(self):
        from miniworld_amd.objmesh import ObjMesh
        out = {}
        for name in [str(m) for m in self.sc["mesh_names"]]:
            m = ObjMesh.get(name)
            out[name] = {"verts": m.verts, "norms": m.norms, "texcs": m.texcs, "colors": m.colors}
        return out

    # ------------------------------------------------------------------ records and writes
    def record(self):
        """Everything that decides the env's future, copied field by field (include/mwengine.h: "record"): the world, the agent,
        the entities as they are and as the last frame showed them, the random stream."""
        d = self.dyn
        return {"sc": self.sc, "dyn_kw": dict(self.dyn_kw), "world_id": self.world_id, "fresh": self.fresh,
                "ag": C.string_at(C.addressof(d.ag), C.sizeof(d.ag)), "ents": C.string_at(d.ents, C.sizeof(d.ents)),
                "render_ents": C.string_at(d.render_ents, C.sizeof(d.render_ents)),
                "rng": None if self.h is None else copy.deepcopy(self.h.np_random.bit_generator.state)}

    def restore(self, rec):
        import pyoracle
        self.sc, self.dyn_kw, self.world_id, self.fresh = rec["sc"], dict(rec["dyn_kw"]), rec["world_id"], rec["fresh"]
        self.dyn = d = pyoracle.Dynamics(self.sc, self.task, **self.dyn_kw)
        C.memmove(C.addressof(d.ag), rec["ag"], C.sizeof(d.ag))
        C.memmove(d.ents, rec["ents"], C.sizeof(d.ents))
        C.memmove(d.render_ents, rec["render_ents"], C.sizeof(d.render_ents))
        if rec["rng"] is not None:
            self.h.np_random.bit_generator.state = copy.deepcopy(rec["rng"])

    WRITABLE = ("agent_pos", "agent_dir", "carrying", "step_count", "ent_pos", "ent_dir")

    def write(self, **fields):
        """mw_set_state's mid-episode injection: the fields given are stored, no consistency is made between them."""
        d = self.dyn
        for name, val in fields.items():
            if name == "agent_pos":
                d.ag.pos[:] = [float(x) for x in val]
            elif name == "agent_dir":
                d.ag.dir = float(val)
            elif name == "carrying":
                d.ag.carrying = int(val)
            elif name == "step_count":
                d.ag.step_count = int(val)
            elif name == "ent_pos":
                for k in range(self.E):
                    d.ents[k].pos[:] = [float(x) for x in val[k]]
            elif name == "ent_dir":
                for k in range(self.E):
                    d.ents[k].dir = float(val[k])
            else:
                raise ValueError(f"write: {name!r} is not modelled; have {self.WRITABLE}")
        # the state is no longer the one reset() built or the last frame showed
        self.fresh = False
        C.memmove(d.render_ents, d.ents, C.sizeof(d.ents))

    def free_for_agent(self, x, z):
        """the oracle's own intersect (miniworld.py:951-961) for the agent standing at (x, z): nothing in the way"""
        return self.dyn.intersect(-1, float(x), float(z), float(self.dyn.ag.radius)) == 0

    def free_for_entity(self, k, x, z):
        return self.dyn.intersect(int(k), float(x), float(z), float(self.dyn.ents[k].radius)) == 0


class ModelSnapshot:
    """save_state()'s records: `records[k]` a ModelEnv.record() (None: never written), `frames[k]` None or (obs, depth, stack)."""

    def __init__(self, capacity, with_frames):
        self.capacity, self.count, self.with_frames = int(capacity), 0, bool(with_frames)
        self.records, self.frames = [None] * capacity, [None] * capacity


class ModelVec:
    """The batch: MiniWorldVecEnv's calls and attributes on numpy arrays.  Every call loops over the envs."""

    def __init__(self, cls, num_envs, seed=0, task=1, domain_rand=False, want_depth=False, autoreset="same_step", final_obs=False,
                 frame_stack=None, stack_pad="reset", **env_kwargs):
        assert autoreset in ("same_step", "next_step", "seeds", "off")
        assert not final_obs or autoreset in ("same_step", "seeds")
        self.N, self.mode, self.K, self.pad = num_envs, autoreset, frame_stack, stack_pad
        self._seed = int(seed)
        # (the engine's env i is created unseeded and reset() seeds it; nothing is observable before reset())
        self.envs = [ModelEnv(cls, self._seed + i, domain_rand, task, **env_kwargs) for i in range(num_envs)]
        h = self.envs[0].h
        self.W, self.H = int(h.obs_width), int(h.obs_height)
        N, H, W = num_envs, self.H, self.W
        self.obs = np.zeros((N, H, W, 3), np.uint8)
        self.depth = np.zeros((N, H, W, 1), np.float32) if want_depth else None
        self.reward = np.zeros(N, np.float32)
        self.terminated, self.truncated = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        self.substeps = np.zeros(N, np.int32)
        self.step_rewards = self.trace = None
        self.pending = np.zeros(N, np.uint8)
        self.final_obs = np.zeros_like(self.obs) if final_obs else None
        self.final_depth = np.zeros_like(self.depth) if final_obs and want_depth else None
        self.stack = [[np.zeros((H, W, 3), np.uint8)] * frame_stack for _ in range(N)] if frame_stack else None
        self.final_stack = np.zeros((N, frame_stack, H, W, 3), np.uint8) if frame_stack and final_obs else None
        self.episode_seed = self.next_seed = None
        if autoreset == "seeds":
            self.episode_seed = np.arange(N, dtype=np.int64) + self._seed
            self.next_seed = np.arange(N, 2 * N, dtype=np.int64) + self._seed
        self._frames, self._meshes = {}, {}
        # bookkeeping of what a run met (the fuzzer's coverage conditions)
        self.cov = dict(ends=0, early_ends=0, loads_on_moved=0, hit_pending=0, hit_carrying=0, hit_after_pickup=0, revisits=0,
                        identical=0, frames=0)
        self._after_pickup = np.zeros(N, bool)
        # mw_get_frame_clean: the byte of the last step, cleared for the envs a load or a state write meets; `clean_known`: 0 where
        # the header promises nothing (an env reset since its last step).  `_left`: an entity left the env's list behind its last frame
        self.clean, self.clean_known, self._left = np.zeros(N, np.uint8), np.ones(N, bool), np.zeros(N, bool)
        self._last_key = [None] * N
        self._recent = [[] for _ in range(N)]

    # ------------------------------------------------------------------ frames
    def _render(self, env, scene, key):
        """pyoracle.render of the scene; a frame is a pure function of the state, so equal states share one drawing"""
        import pyoracle
        if key not in self._frames:
            for name, arrs in env.meshes().items():
                self._meshes.setdefault(name, arrs)
            out = pyoracle.render(scene, width=self.W, height=self.H, meshes=self._meshes)
            self._frames[key] = (out["rgb"], out["depth"])
        return self._frames[key]

    def _show(self, i, frame):
        self.obs[i] = frame[0]
        if self.depth is not None:
            self.depth[i] = frame[1]

    def _rebuild(self, i):
        """a new episode's stack: K copies of its first frame, or K - 1 all-zero frames and the frame"""
        if self.K:
            f = self.obs[i].copy()
            self.stack[i] = [f if self.pad == "reset" else np.zeros_like(f)] * (self.K - 1) + [f]

    def _push(self, i):
        if self.K:
            self.stack[i] = self.stack[i][1:] + [self.obs[i].copy()]

    def _redraw(self, rebuilt=()):
        """mw_render + mw_stack_refresh: every env's frame drawn from its state as it is now; the stacks of the envs whose world a
        reset or a load wrote since their last push rebuilt, every other stack left alone"""
        for i, e in enumerate(self.envs):
            self._show(i, self._render(e, e.scene_now(), e.key()))
        for i in rebuilt:
            self._rebuild(i)
        return self.obs

    def stack_array(self):
        return None if not self.K else np.array(self.stack)

    # ------------------------------------------------------------------ reset
    def reset(self, seed=None):
        if seed is not None:
            self._seed = int(seed)
        s, N = self._seed, self.N
        if self.mode == "seeds":
            self.episode_seed[:] = np.arange(s, s + N)
            self.next_seed[:] = np.arange(s + N, s + 2 * N)
        self._seed += N
        for i, e in enumerate(self.envs):
            e.reset(s + i)
        self.pending[:] = 0
        self.clean_known[:], self._left[:] = False, False
        self._touched(range(N), count=False)
        return self._redraw(range(N))

    def reset_where(self, mask, seeds):
        hit = [i for i in range(self.N) if mask[i]]
        self._touched(hit)
        for i in hit:
            self.envs[i].reset(int(seeds[i]))
            self.pending[i] = 0
            self.clean_known[i], self._left[i] = False, False
            if self.episode_seed is not None:
                self.episode_seed[i] = int(seeds[i])
        return self._redraw(hit)

    # ------------------------------------------------------------------ steps
    def step(self, actions, repeat=1):
        self._advance(np.repeat(np.asarray(actions)[None], repeat, 0), None, None)
        return self.obs, self.reward, self.terminated, self.truncated

    TRACE_DEFAULT = ("agent_pos", "agent_dir", "carrying")

    def rollout(self, plans, trace=None, trace_ent=None):
        names = None if trace in (None, False) else self.TRACE_DEFAULT if trace is True else tuple(trace)
        slot = self.envs[0].dyn_kw["goal_ent"] if trace_ent is None else trace_ent
        self._advance(np.asarray(plans), names, slot)
        return self.obs, self.reward, self.terminated, self.truncated

    def _trace_row(self, e, slot):
        ag = e.dyn.ag
        return {"agent_pos": np.array(ag.pos[:]), "agent_dir": float(ag.dir), "carrying": int(ag.carrying),
                "ent_pos": np.array(e.dyn.ents[slot or 0].pos[:])}

    def _advance(self, plans, names, slot):
        """`for k in range(T): step(plans[k][i]); if done: break`, then the auto-reset of the mode, one frame, one push"""
        T, N = plans.shape
        self.step_rewards = np.zeros((T, N), np.float32)
        rows = [[None] * N for _ in range(T)]
        for i, e in enumerate(self.envs):
            self._after_pickup[i] = False
            if self.mode == "next_step" and self.pending[i]:
                # the reset step: the action is ignored, no draws, reward 0, no flags; the next world of the env's own stream
                for k in range(T):
                    rows[k][i] = self._trace_row(e, slot)
                e.reset()
                self.pending[i] = 0
                self.clean[i], self.clean_known[i], self._left[i] = 0, True, False
                self.reward[i], self.terminated[i], self.truncated[i], self.substeps[i] = 0.0, 0, 0, 0
                self._show(i, self._render(e, e.frame_scene(), e.frame_key()))
                self._rebuild(i)
                self._seen(i, e)
                continue
            total, te, tr, n = 0.0, False, False, 0
            unchanged = True
            for k in range(T):
                alive0 = sum(bool(e.dyn.ents[j].alive) for j in range(e.E))
                before = self._clean_key(e)
                r, te, tr = e.substep(int(plans[k, i]))
                self._after_pickup[i] = sum(bool(e.dyn.ents[j].alive) for j in range(e.E)) < alive0
                # frame clean: pose, carried slot and the carried entity's pose as they were, no entity leaves or has just left
                unchanged &= before == self._clean_key(e) and not self._after_pickup[i] and not self._left[i]
                self._left[i] = self._after_pickup[i]
                total += r                                  # (in double, in order)
                self.step_rewards[k, i] = np.float32(r)
                rows[k][i] = self._trace_row(e, slot)
                n += 1
                if te or tr:
                    break
            for k in range(n, T):
                rows[k][i] = rows[n - 1][i]
            self.reward[i], self.terminated[i], self.truncated[i], self.substeps[i] = np.float32(total), te, tr, n
            frame = self._render(e, e.frame_scene(), e.frame_key())
            self._seen(i, e)
            done = te or tr
            installs = done and self.mode in ("same_step", "seeds")
            self.clean[i], self.clean_known[i] = unchanged and not installs, True
            if installs:
                self._left[i] = False
            if done:
                self.cov["ends"] += 1
                self.cov["early_ends"] += n < T
                self._after_pickup[i] = False
            if done and self.mode in ("same_step", "seeds"):
                if self.final_obs is not None:
                    self.final_obs[i] = frame[0]
                    if self.final_depth is not None:
                        self.final_depth[i] = frame[1]
                    if self.final_stack is not None:
                        self.final_stack[i] = np.array(self.stack[i][1:] + [frame[0]])
                if self.mode == "seeds":
                    # the caller's writes win: next_seed is read now, for this env alone
                    e.reset(int(self.next_seed[i]))
                    self.episode_seed[i] = self.next_seed[i]
                    self.next_seed[i] += N
                else:
                    e.reset()
                self._show(i, self._render(e, e.frame_scene(), e.frame_key()))
                self._rebuild(i)
                self._seen(i, e)
                continue
            if done and self.mode == "next_step":
                self.pending[i] = 1
            self._show(i, frame)
            self._push(i)
        self.trace = None if names is None else {name: np.array([[rows[k][i][name] for i in range(N)] for k in range(T)]) for name in names}

    @staticmethod
    def _clean_key(e):
        ag = e.dyn.ag
        c = e.dyn.ents[ag.carrying] if ag.carrying >= 0 else None
        return (bytes(ag.pos), float(ag.dir), int(ag.carrying), None if c is None else (bytes(c.pos), float(c.dir)))

    def _seen(self, i, e):
        """coverage: is the frame the env's last one again, or one of its last four distinct ones (counted on the states)"""
        key = e.frame_key()
        self.cov["frames"] += 1
        if key == self._last_key[i]:
            self.cov["identical"] += 1
        elif key in self._recent[i]:
            self.cov["revisits"] += 1
        if key in self._recent[i]:
            self._recent[i].remove(key)
        self._recent[i] = (self._recent[i] + [key])[-4:]
        self._last_key[i] = key

    def _touched(self, envs, count=True):
        """coverage: a load, reset_where or state write meets these envs"""
        for i in envs:
            if count:
                self.cov["hit_pending"] += int(self.pending[i])
                self.cov["hit_carrying"] += self.envs[i].dyn.ag.carrying >= 0
                self.cov["hit_after_pickup"] += bool(self._after_pickup[i])
        self._after_pickup[:] = False

    # ------------------------------------------------------------------ save / load / fork
    def _frame_record(self, i):
        return (self.obs[i].copy(), None if self.depth is None else self.depth[i].copy(), None if not self.K else list(self.stack[i]))

    def save_state(self, envs=None, capacity=None, frames=False, into=None, records=None):
        envs = list(range(self.N)) if envs is None else [int(i) for i in envs]
        if into is None:
            snap = ModelSnapshot(len(envs) if capacity is None else capacity, frames)
            records = range(len(envs))
        else:
            snap = into
        for i, k in zip(envs, records):
            snap.records[k] = dict(self.envs[i].record(), pending=int(self.pending[i]), left=bool(self._left[i]))
            snap.frames[k] = self._frame_record(i) if snap.with_frames else None
            snap.count = max(snap.count, int(k) + 1)
        return snap

    def _load(self, pairs, snap, frames):
        """env i := record k for (i, k) in pairs; with frames the rows the record holds, else a redraw and new stacks"""
        if frames is None:
            frames = snap.with_frames
        assert not frames or snap.with_frames
        pairs = [(int(i), int(k)) for i, k in pairs]
        for i, k in pairs:
            self.cov["loads_on_moved"] += self.envs[i].key() != (snap.records[k]["world_id"], snap.records[k]["ag"][:24],
                                                                 snap.records[k]["ag"][24:32], snap.records[k]["ents"])
        self._touched([i for i, _ in pairs])
        for i, k in pairs:
            rec = snap.records[k]
            self.envs[i].restore(rec)
            self.pending[i], self._left[i] = rec["pending"], rec["left"]
            self.clean[i], self.clean_known[i] = 0, True
            if frames:
                obs, depth, stack = snap.frames[k]
                self.obs[i] = obs
                if self.depth is not None:
                    self.depth[i] = depth
                if self.K:
                    self.stack[i] = list(stack)
        return self.obs if frames else self._redraw([i for i, _ in pairs])

    def load_state(self, snap, envs=None, records=None, frames=None):
        n = len(envs) if envs is not None else len(records) if records is not None else min(snap.count, self.N)
        envs = range(n) if envs is None else envs
        records = range(n) if records is None else records
        return self._load(list(zip(envs, records)), snap, frames)

    def load_state_where(self, snap, mask, records, frames):
        """the masked form (mw_snapshot_load_where, and its frame twin or a redraw behind it)"""
        return self._load([(i, records[i]) for i in range(self.N) if mask[i]], snap, frames)

    def fork(self, src, frames=False):
        snap = self.save_state(frames=frames)
        return self._load(list(zip(range(self.N), src)), snap, frames)

    # ------------------------------------------------------------------ state views
    def set_state_where(self, mask, **fields):
        hit = [i for i in range(self.N) if mask[i]]
        self._touched(hit)
        for i in hit:
            self.envs[i].write(**{name: val[i] for name, val in fields.items()})
            self.pending[i] = 0         # (and with it the stack rebuild that reset would have caused; the stacks stay)
            self.clean[i], self.clean_known[i] = 0, True
        return self._redraw()

    def state(self):
        """the default fields of MiniWorldVecEnv.state(), `alive` in the place of ent_kind"""
        rows = [e.state() for e in self.envs]
        return {"agent_pos": np.array([r[0] for r in rows]), "agent_dir": np.array([r[1] for r in rows]),
                "carrying": np.array([r[2] for r in rows], np.int32), "step_count": np.array([r[3] for r in rows], np.int32),
                "alive": [r[4] for r in rows], "ent_pos": [r[5] for r in rows], "ent_dir": [r[6] for r in rows]}

    def reset_pending(self):
        return self.pending.copy()
