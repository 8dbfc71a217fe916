"""What the "levels" and "seeds" auto-reset modes do behind a step and at reset, with no host value: the bank finished envs restart
from (set_levels) and the seeds the device holds.  `Restarts` is a mixin of MiniWorldVecEnv (vec_env.py)."""
from __future__ import annotations

from ._args import on_device


class Restarts:
    def _advance_seeds(self):
        """behind a step in seed mode, with no host value: episode_seed follows the envs that finished, their next_seed moves N on"""
        torch = self.torch
        torch.bitwise_or(self.terminated, self.truncated, out=self._done)
        torch.ne(self._done, 0, out=self._done_b)
        torch.where(self._done_b, self.next_seed, self.episode_seed, out=self.episode_seed)
        self._done_i.copy_(self._done_b)
        self.next_seed.add_(self._done_i, alpha=self.num_envs)

    def set_levels(self, snap, generator=None):
        """autoreset="levels": `snap` (make_levels, or any snapshot with frame records of this env's frame configuration) becomes the
        bank finished envs restart from; its buffers are moved to the device once.  Creates `self.level` and `self.next_level`, int32[N]
        on the device: level[i] is the record env i is playing (`self.played_level`: the one it played in the step that just ended,
        which differs for the envs that step finished), next_level[i] the one it gets when its episode ends — drawn uniformly
        from 0 .. len(snap) - 1 with torch.randint(generator=generator) behind every step, and the caller's to overwrite between
        steps (a level-replay sampler writes its choice there, on the device).  Call reset() next."""
        torch = self.torch
        if self.autoreset_mode != "levels":
            raise RuntimeError(f"set_levels needs autoreset='levels' (this env: {self.autoreset_mode!r})")
        self._check_frame_config(snap, "set_levels")
        if snap.count < 1:
            raise ValueError("set_levels: the snapshot holds no records")
        dev, N = self.engine.device, self.num_envs
        self.levels = snap if on_device(snap, dev) else snap.to(dev)
        self._level_gen = generator
        self.level, self.next_level, self.played_level = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(3))
        self._done_scratch()
        self._ones = torch.ones(N, dtype=torch.uint8, device=dev)
        self._draw_next_levels()

    def _need_levels(self, what):
        if self.levels is None:
            raise RuntimeError(f"{what}() with autoreset='levels' before set_levels(): there is no bank to restart finished envs from")

    def _draw_next_levels(self):
        self.torch.randint(0, self.levels.count, (self.num_envs,), generator=self._level_gen, out=self.next_level)

    def _start_levels(self, mask, frames):
        """the envs under `mask` (uint8[N], device) start level next_level[i]: states, then frames; then the bookkeeping"""
        torch, bank = self.torch, self.levels
        self.engine.snapshot_load_where(bank.data, bank.count, bank.capacity, mask, self.next_level)
        if frames:
            self.engine.snapshot_load_frames_where(bank.frames, bank.count, bank.capacity, mask, self.next_level, self.obs, self.depth, bank.frame_flags)
        torch.ne(mask, 0, out=self._done_b)
        self.played_level.copy_(self.level)
        torch.where(self._done_b, self.next_level, self.level, out=self.level)
        self._draw_next_levels()

    def _finished_to_levels(self, frames):
        """behind a step in level mode, with no host synchronisation: done, the terminal infos, the two loads, level, next_level"""
        torch = self.torch
        torch.bitwise_or(self.terminated, self.truncated, out=self._done)
        if self._info_kind is not None:
            # the finished episodes' own values, before the loads replace the states they are read from (final_infos)
            now = self.infos()[self._info_kind]
            kept = self._info_buffer("_final_info_buf")
            done = self._done.bool()
            torch.where(done if now.dim() == 1 else done[:, None], now, kept, out=kept)
        self._start_levels(self._done, frames)

