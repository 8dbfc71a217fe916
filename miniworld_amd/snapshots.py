"""Records of env states (EnvSnapshot) and what MiniWorldVecEnv does with them: save_state, load_state, fork, and make_levels, which
builds a bank of levels out of them.  `Snapshots` is a mixin of MiniWorldVecEnv (vec_env.py): it uses the env's engine, buffers and
_redraw()."""
from __future__ import annotations

import numpy as np

from . import engine as eng
from ._args import on_device, seeds_u64


class EnvSnapshot:
    """Records of MiniWorldVecEnv.save_state(): `data`, the engine's opaque uint8 record buffer (a torch tensor; its header carries
    the layout key of the configuration it was taken under), `count`, the valid records, and `capacity`, the records the buffer was
    laid out for.  A snapshot taken with frames=True also holds `frames`, the engine's frame record buffer (the observation, depth
    and stacked frames each env had at the save), `frame_flags`, the engine.SNAPF_* bits it was saved under, and `frame_stack`, the
    stack depth K of its stacks (0: none); without frames they are None, 0 and 0.  `.cpu()` / `.to(device)` move it, so
    `torch.save(snap.cpu().state_dict(), path)` and `EnvSnapshot.from_state_dict(torch.load(path))` write a checkpoint and read it
    back.  A bank of levels (MiniWorldVecEnv.make_levels) also carries `seeds`, the int64 tensor of the seed each record was reset
    with; None otherwise."""

    def __init__(self, data, count: int, capacity: int, frames=None, frame_flags: int = 0, frame_stack: int = 0, seeds=None):
        self.data, self.count, self.capacity = data, int(count), int(capacity)
        self.frames = frames
        self.frame_flags, self.frame_stack = (int(frame_flags), int(frame_stack)) if frames is not None else (0, 0)
        self.seeds = seeds

    def _with(self, move):
        return EnvSnapshot(move(self.data), self.count, self.capacity, None if self.frames is None else move(self.frames),
                           self.frame_flags, self.frame_stack, None if self.seeds is None else move(self.seeds))

    def to(self, device):
        return self._with(lambda t: t.to(device))

    def cpu(self):
        return self.to("cpu")

    def clone(self):
        return self._with(lambda t: t.clone())

    def state_dict(self):
        d = {"data": self.data, "count": self.count, "capacity": self.capacity}
        if self.frames is not None:
            d.update(frames=self.frames, frame_flags=self.frame_flags, frame_stack=self.frame_stack)
        if self.seeds is not None:
            d.update(seeds=self.seeds)
        return d

    @classmethod
    def from_state_dict(cls, d):
        return cls(d["data"], d["count"], d["capacity"], d.get("frames"), d.get("frame_flags", 0), d.get("frame_stack", 0), d.get("seeds"))

    def __len__(self):
        return self.count


class Snapshots:
    def make_levels(self, seeds):
        """A bank of levels: record l of the returned EnvSnapshot IS the reference's env.reset(seed=seeds[l]) on the PCG64 stream —
        world, agent, random stream, pre-generated next world — together with its first observation (depth, frame stack) as frame
        records under this env's frame flags.  `seeds` is an integer sequence or tensor of any length L, more than num_envs too: the
        bank is built num_envs levels at a time (engine.reset with the seeds, a render, a stack refresh, then mw_snapshot_save_at /
        mw_snapshot_save_frames_at into records base .. base + m - 1).  `snap.seeds` keeps the seeds (int64).
        Afterwards this env's own state is the last chunk's: call reset() or set_levels() next.
        A record carries the env's random stream, so under domain randomisation every replay of a level draws the same per-step
        noise; a bank that keeps the level but not the stream is not built here."""
        torch = self.torch
        seeds_np = seeds.detach().cpu().numpy() if isinstance(seeds, torch.Tensor) else np.asarray(seeds)
        if seeds_np.ndim != 1 or seeds_np.size == 0 or seeds_np.dtype.kind not in "iu":
            raise ValueError(f"make_levels: seeds: need a non-empty 1-D integer sequence, got {seeds_np.dtype} {seeds_np.shape}")
        seeds_np = seeds_u64("make_levels", seeds_np)
        L, N, dev = int(seeds_np.size), self.num_envs, self.engine.device
        flags = self._frame_flags()
        data = torch.zeros(self.engine.snapshot_bytes(L), dtype=torch.uint8, device=dev)
        fdata = torch.zeros(self.engine.snapshot_frames_bytes(L, flags), dtype=torch.uint8, device=dev)
        for base in range(0, L, N):
            m = min(N, L - base)
            mask, full = np.zeros(N, np.uint8), np.zeros(N, np.uint64)
            mask[:m], full[:m] = 1, seeds_np[base:base + m]
            self.engine.reset(mask, full)
            self._redraw()
            recs = torch.arange(base, base + m, dtype=torch.int32, device=dev)     # (envs None: env k is item k, k < m)
            self.engine.snapshot_save_at(data, L, None, recs)
            self.engine.snapshot_save_frames_at(fdata, L, self.obs, self.depth, flags, None, recs)
        return EnvSnapshot(data, L, L, fdata, flags, self.frame_stack or 0, torch.from_numpy(seeds_np.astype(np.int64)).to(dev))

    def _check_frame_config(self, snap, what):
        if snap.frames is None:
            raise ValueError(f"{what}: the snapshot holds no frame records (make_levels, save_state(frames=True))")
        if snap.frame_flags != self._frame_flags() or snap.frame_stack != (self.frame_stack or 0):
            raise ValueError(f"{what}: the snapshot's frame records (flags {snap.frame_flags}, frame_stack {snap.frame_stack}) are not this "
                             f"env's (flags {self._frame_flags()}, frame_stack {self.frame_stack or 0}: want_depth / frame_stack differ)")

    def save_state(self, envs=None, capacity: int | None = None, frames: bool = False, into=None, records=None):
        """The complete state of the envs `envs` (an integer sequence or tensor; None: all of them, in order) as an EnvSnapshot on
        the device: everything that decides their future — poses, entities, step counts, the random stream, pending removals and
        resets, the Maze's own geometry, the pre-generated next world — but no frames (include/mwengine.h: mw_snapshot_save).  One
        kernel on the current stream; nothing in this env changes.
        capacity: the records the buffer is laid out for (default: the number saved).  One load_state call moves at most that many
        envs, so a snapshot of ONE state that is to be loaded into many envs at once ("reset all of them to this cell") is taken
        with capacity=num_envs: `vec.load_state(vec.save_state([i], capacity=n), records=torch.zeros(n, dtype=torch.int32))`.
        frames=True: a second kernel also saves what the agent saw — the envs' rows of `self.obs`, of `self.depth` with want_depth,
        and their frame stacks with frame_stack (mw_snapshot_save_frames) — into `snap.frames`; load_state() then puts those
        frames back instead of drawing new ones.
        into=snap, records=idx: the envs are saved into the records idx[k] (distinct) of an EXISTING snapshot on this env's device
        instead (mw_snapshot_save_at), their frames too when `snap` has frame records — they must be of this env's frame
        configuration —, and `snap` is returned; its other records keep what they held and its count grows to cover the highest
        record named.  A running loop adds states to a bank this way: an archive of cells, a curriculum of reached states.
        ValueError for a snapshot of another frame configuration, for indices of the wrong length, and for `into` with `capacity`."""
        torch = self.torch
        if into is not None:
            return self._save_into(into, envs, records, capacity)
        if records is not None:
            raise ValueError("save_state: records needs into=<snapshot>")
        envs, count = self._named_envs(envs)
        capacity = count if capacity is None else int(capacity)
        if capacity < count:
            raise ValueError(f"capacity {capacity} < the {count} records to save")
        data = torch.zeros(self.engine.snapshot_bytes(capacity), dtype=torch.uint8, device=self.engine.device)
        self.engine.snapshot_save(data, capacity, envs)
        if not frames:
            return EnvSnapshot(data, count, capacity)
        flags = self._frame_flags()
        fdata = torch.zeros(self.engine.snapshot_frames_bytes(capacity, flags), dtype=torch.uint8, device=self.engine.device)
        self.engine.snapshot_save_frames(fdata, capacity, self.obs, self.depth, flags, envs)
        return EnvSnapshot(data, count, capacity, fdata, flags, self.frame_stack or 0)

    def _named_envs(self, envs):
        """(the envs a save names, as a tensor or None for all of them in order; how many they are)"""
        envs = None if envs is None else self.torch.as_tensor(envs)
        return envs, self.num_envs if envs is None else int(envs.numel())

    def _save_into(self, snap, envs, records, capacity):
        torch = self.torch
        if capacity is not None:
            raise ValueError("save_state: into=<snapshot> has its own capacity; capacity cannot be given with it")
        if records is None:
            raise ValueError("save_state: into=<snapshot> needs records=<the record indices>")
        if snap.frames is not None:
            self._check_frame_config(snap, "save_state(into=...)")
        envs, count = self._named_envs(envs)
        rec_host = torch.as_tensor(records)
        if rec_host.dim() != 1 or int(rec_host.numel()) != count:
            raise ValueError(f"save_state: {tuple(rec_host.shape)} record indices for {count} envs")
        if count > snap.capacity:
            raise ValueError(f"save_state: {count} records into a snapshot of capacity {snap.capacity}")
        if not on_device(snap, self.engine.device):
            raise ValueError(f"save_state: into=<snapshot> must live on {self.engine.device} (snap.to(device))")
        envs, recs = self.engine._index_tensor(envs, "envs"), self.engine._index_tensor(records, "records")
        self.engine.snapshot_save_at(snap.data, snap.capacity, envs, recs)
        if snap.frames is not None:
            self.engine.snapshot_save_frames_at(snap.frames, snap.capacity, self.obs, self.depth, snap.frame_flags, envs, recs)
        if rec_host.device.type == "cpu" and count:     # (device indices: the caller keeps count; nothing is read back here)
            snap.count = max(snap.count, min(int(rec_host.max()) + 1, snap.capacity))
        return snap

    def _frame_flags(self):
        """the engine.SNAPF_* bits of this env's frame records: depth with want_depth, the stacks with frame_stack"""
        return (eng.SNAPF_DEPTH if self.depth is not None else 0) | (eng.SNAPF_STACK if self.frame_stack else 0)

    def load_state(self, snap, envs=None, records=None, frames: bool | None = None):
        """Env envs[k] becomes record records[k] of `snap` (envs=None: env k; records=None: record k; the envs must be distinct,
        records may repeat; one call moves at most `snap.capacity` envs) and continues bit for bit as the env the record was taken from would have — on this env or on another
        one of the same configuration, whatever its num_envs.  Draws the new frames (and rebuilds the loaded envs' frame stacks as
        reset() does) and returns `self.obs`; rewards and flags are left alone.
        frames: None uses the snapshot's frame records if it has any (save_state(frames=True)), False never does, True insists
        (ValueError without them).  With them nothing is drawn and no stack is rebuilt: the loaded envs' rows of `self.obs` /
        `self.depth` and their stacks are copied back (mw_snapshot_load, mw_snapshot_load_frames).  What differs from the redraw:
        the observation is the one the record's source RETURNED — a picked-up object's last appearance included, which a frame of
        the restored state does not show — and `self.stack` is the source's stack, not a new episode's.  The snapshot's frame flags
        and stack depth must be this env's (want_depth, frame_stack): ValueError otherwise, before anything is launched."""
        if frames is None:
            frames = snap.frames is not None
        if frames:
            self._check_frame_config(snap, "load_state")
        if not on_device(snap, self.engine.device):
            snap = snap.to(self.engine.device)
        if frames:      # (both loads take the same indices: made device tensors once)
            envs, records = self.engine._index_tensor(envs, "envs"), self.engine._index_tensor(records, "records")
        self.engine.snapshot_load(snap.data, snap.count, snap.capacity, envs, records)
        if not frames:
            return self._redraw()
        self.engine.snapshot_load_frames(snap.frames, snap.count, snap.capacity, self.obs, self.depth, snap.frame_flags, envs, records)
        return self.obs

    def fork(self, src, frames: bool = False):
        """src: integer tensor [N].  Env j becomes a copy of env src[j] (its stream included: copies given the same actions stay
        identical) — a whole-batch save into scratch records of this env's own and a load through `src`, two kernels and a frame;
        returns `self.obs`.
        frames=True: no frame is drawn.  Env j's frame after the fork IS env src[j]'s, and it is already on the device: the frames
        are saved and loaded through `src` like the states — save, save_frames, load, load_frames, four copy kernels.  What differs
        from the redraw: env j's observation (and depth) is the one env src[j]'s last step returned — a picked-up object's last
        appearance included — and its frame stack is env src[j]'s, so a policy that reads `self.stack` sees in the copy what it saw
        in the source."""
        eng_ = self.engine
        n = self.num_envs
        if self._fork_buf is None:
            self._fork_buf = self.torch.empty(eng_.snapshot_bytes(n), dtype=self.torch.uint8, device=eng_.device)
        src = eng_._index_tensor(src, "src", n)
        flags = self._frame_flags()
        if frames and self._fork_frames is None:
            self._fork_frames = self.torch.empty(eng_.snapshot_frames_bytes(n, flags), dtype=self.torch.uint8, device=eng_.device)
        eng_.snapshot_save(self._fork_buf, n)
        if frames:
            eng_.snapshot_save_frames(self._fork_frames, n, self.obs, self.depth, flags)
        eng_.snapshot_load(self._fork_buf, n, n, None, src)
        if not frames:
            return self._redraw()
        eng_.snapshot_load_frames(self._fork_frames, n, n, self.obs, self.depth, flags, None, src)
        return self.obs
