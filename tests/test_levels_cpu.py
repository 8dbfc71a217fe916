"""Level sets (mw_snapshot_save_at / mw_snapshot_save_frames_at / mw_snapshot_load_where / mw_snapshot_load_frames_where), host side,
without a GPU: the header declares the four with their signatures and says what a masked load owes the other envs, the ABI version did
not move, the library exports them and refuses a null engine, the policy's decisions for them (miniworld_amd/csrc/mw_policy.h, compiled
for the host from tests/hostcheck/levels_policy.cpp) are the documented ones, and MiniWorldVecEnv's level mode checks its arguments and
reaches the entry points in the documented order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_launch_policy_cpu import policy_lib
from helpers import stub_engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "levels_policy.cpp")
LIB = os.path.join(HERE, "hostcheck", "libmwlevels.so")
NAMES = ("mw_snapshot_save_at", "mw_snapshot_save_frames_at", "mw_snapshot_load_where", "mw_snapshot_load_frames_where")
SNAPF_DEPTH, SNAPF_STACK = 1, 2


def _ask(what, args, n):
    lib = policy_lib(SRC, LIB)          # (the build rule, the dependencies and the entry point's name of tests/hostcheck/policy.cpp)
    a, out = np.array(list(args) + [0], np.int64), np.zeros(8, np.int64)
    assert lib.mwpol(what, a.ctypes.data, out.ctypes.data) == n
    return out[:n].tolist()


def test_header_declares_the_entry_points():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_snapshot_save_at\(mw_engine \*e, const int32_t \*d_envs, const int32_t \*d_recs, int32_t count,\s*"
                     r"uint8_t \*d_snap, int32_t capacity, void \*stream\);", header)
    assert re.search(r"int mw_snapshot_save_frames_at\(mw_engine \*e, const int32_t \*d_envs, const int32_t \*d_recs, int32_t count,\s*"
                     r"const uint8_t \*d_obs, const float \*d_depth, uint8_t \*d_frames,\s*int32_t capacity, int32_t flags, void \*stream\);", header)
    assert re.search(r"int mw_snapshot_load_where\(mw_engine \*e, const uint8_t \*d_mask, const int32_t \*d_recs, const uint8_t \*d_snap,\s*"
                     r"int32_t n_recs, int32_t capacity, void \*stream\);", header)
    assert re.search(r"int mw_snapshot_load_frames_where\(mw_engine \*e, const uint8_t \*d_mask, const int32_t \*d_recs, const uint8_t \*d_frames,\s*"
                     r"int32_t n_recs, int32_t capacity, int32_t flags, uint8_t \*d_obs, float \*d_depth,\s*void \*stream\);", header)
    # what the masked loads owe the envs they do not write, and the frame that frame reuse holds
    text = " ".join(header.split())
    assert "leaves the other envs' cached frames alone" in text
    assert "drop the held frame" in text
    # the list forms are declared as they were
    assert re.search(r"int mw_snapshot_load\(mw_engine \*e, const int32_t \*d_envs, const int32_t \*d_recs, int32_t count,\s*"
                     r"const uint8_t \*d_snap, int32_t n_recs, int32_t capacity, void \*stream\);", header)


def test_library_exports_the_entry_points_and_refuses_a_null_engine():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    buf, obs, mask = (C.c_uint8 * 256)(), (C.c_uint8 * 64)(), (C.c_uint8 * 4)(1, 1, 1, 1)
    recs = (C.c_int32 * 4)()
    p, o, m, r = (C.cast(x, C.c_void_p) for x in (buf, obs, mask, recs))
    assert lib.mw_snapshot_save_at(None, None, r, 1, p, 4, None) == -1           # no engine: MW_E_INVALID
    assert lib.mw_snapshot_save_frames_at(None, None, r, 1, o, None, p, 4, 0, None) == -1
    assert lib.mw_snapshot_load_where(None, m, r, p, 1, 4, None) == -1
    assert lib.mw_snapshot_load_frames_where(None, m, r, p, 1, 4, 0, o, None, None) == -1
    assert not any(buf) and not any(obs)
    assert lib.mw_abi_version() == 4


def test_what_a_load_invalidates():
    """A list load marks every env's cached frames dirty, a masked load does not (its kernel advances the epochs of the envs it
    writes); both drop the held frame, and so do the frame loads, which never touch the cache."""
    assert _ask(0, [0], 4) == [1, 1, 1, 0]
    assert _ask(0, [1], 4) == [1, 0, 1, 0]


@pytest.mark.parametrize("N,capacity", [(4096, 200), (300, 7), (70, 1), (3, 0), (257, 256)])
def test_the_masked_grid_is_the_list_forms_grid_over_all_envs(N, capacity):
    """N items whatever the capacity is: the capacity is no argument of the grid, and N > capacity is no error of it."""
    assert capacity < N
    for rows, per_item in ((37, 0), (52, 12)):      # shared geometry; per-env geometry sets with blob workgroups
        chunks, blocks, l_chunks, l_blocks = _ask(1, [N, rows, per_item], 4)
        assert (chunks, blocks) == (l_chunks, l_blocks) == (-(-N // 256), -(-N // 256) * rows + N * per_item)
    for bits, fb, db, K in ((0, 14400, 0, 0), (0, 14400, 19200, 4), (0, 81 * 61 * 3, 81 * 61 * 4, 3), (8, 14400, 0, 2)):
        wide, per_item, blocks, l_wide, l_per_item, l_blocks = _ask(2, [bits, fb, db, K, N], 6)
        assert (wide, per_item, blocks) == (l_wide, l_per_item, l_blocks) and blocks == per_item * N
        assert wide == (bits % 16 == 0 and fb % 16 == 0 and db % 16 == 0)


def _names(calls):
    return [c[0] for c in calls if c[0] not in ("mw_snapshot_bytes", "mw_snapshot_frames_bytes")]


def test_level_mode_refuses_on_the_host(monkeypatch):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    with pytest.raises(ValueError, match="terminal frame"):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, autoreset="levels", final_obs=True)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, autoreset="levels", frame_stack=2)
    assert vec.autoreset_mode == "levels" and vec.engine.cfg.autoreset == 0        # MW_AUTORESET_OFF
    acts = torch.zeros(4, dtype=torch.int32)
    n0 = len(lib.calls)
    for call in (lambda: vec.step(acts), lambda: vec.reset(), lambda: vec.rollout(acts[None])):
        with pytest.raises(RuntimeError, match="set_levels"):
            call()
    assert lib.calls[n0:] == []
    # save_state: into excludes capacity, wants as many records as envs, and frame records of this env's configuration
    snap = vec.save_state(capacity=8, frames=True)
    with pytest.raises(ValueError, match="capacity"):
        vec.save_state([0, 1], capacity=8, into=snap, records=[4, 5])
    with pytest.raises(ValueError, match="record indices"):
        vec.save_state([0, 1], into=snap, records=[4, 5, 6])
    other = MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, autoreset="levels", frame_stack=3)
    n0 = len(lib.calls)
    with pytest.raises(ValueError, match="frame"):
        other.save_state([0, 1], into=snap, records=[4, 5])
    # set_levels: other frame flags (K = 2 into K = 3, stacks into an env without one, no frame records at all) before any engine call
    plain = MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, autoreset="levels")
    n0 = len(lib.calls)
    for env, bank in ((other, snap), (plain, snap)):
        with pytest.raises(ValueError):
            env.set_levels(bank)
    assert lib.calls[n0:] == []
    stateless = vec.save_state()
    n0 = len(lib.calls)
    with pytest.raises(ValueError):
        vec.set_levels(stateless)
    assert lib.calls[n0:] == []
    with pytest.raises(RuntimeError):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 4).set_levels(snap)


def test_save_state_into_reaches_the_at_calls(monkeypatch):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, want_depth=True)
    snap = vec.save_state([0], capacity=8, frames=True)
    assert snap.count == 1
    n0 = len(lib.calls)
    assert vec.save_state([3, 1], into=snap, records=torch.tensor([6, 2])) is snap
    assert _names(lib.calls[n0:]) == ["mw_snapshot_save_at", "mw_snapshot_save_frames_at"]
    save, savef = [c[1] for c in lib.calls[n0:] if c[0] in NAMES]
    assert save[1] is not None and save[2] is not None and save[3] == 2 and save[4].value == snap.data.data_ptr() and save[5] == 8
    assert savef[1].value == save[1].value and savef[2].value == save[2].value and savef[3] == 2
    assert savef[4].value == vec.obs.data_ptr() and savef[5].value == vec.depth.data_ptr() and savef[7:9] == (8, SNAPF_DEPTH)
    assert snap.count == 7          # the records up to the highest one named count as valid
    bare = vec.save_state([0], capacity=8)
    n0 = len(lib.calls)
    vec.save_state(into=bare, records=[0, 1, 2, 3])
    assert _names(lib.calls[n0:]) == ["mw_snapshot_save_at"] and lib.calls[-1][1][1] is None and lib.calls[-1][1][3] == 4


def test_make_levels_fills_the_bank_in_chunks(monkeypatch):
    """L = 2.5 N: three chunks — seeded reset, render, stack refresh, the two saves — into records 0 .. 3, 4 .. 7 and 8 .. 9."""
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    resets, saves = [], []
    monkeypatch.setattr(engine.Engine, "reset", lambda self, mask=None, seeds=None: (lib.calls.append(("mw_reset", ())), resets.append((mask.copy(), seeds.copy())))[0])
    real = engine.Engine.snapshot_save_at

    def save_at(self, buf, capacity, envs=None, records=None, count=None):
        saves.append((capacity, envs, records.clone()))
        return real(self, buf, capacity, envs, records, count)
    monkeypatch.setattr(engine.Engine, "snapshot_save_at", save_at)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, autoreset="levels", frame_stack=2)
    seeds = [100 + 3 * k for k in range(10)]
    n0 = len(lib.calls)
    bank = vec.make_levels(seeds)
    chunk = ["mw_reset", "mw_render", "mw_stack_refresh", "mw_snapshot_save_at", "mw_snapshot_save_frames_at"]
    assert _names(lib.calls[n0:]) == chunk * 3
    assert [m.tolist() for m, _ in resets] == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 0, 0]]
    assert [s[:int(m.sum())].tolist() for m, s in resets] == [seeds[0:4], seeds[4:8], seeds[8:10]]
    assert [(c, e, r.tolist()) for c, e, r in saves] == [(10, None, [0, 1, 2, 3]), (10, None, [4, 5, 6, 7]), (10, None, [8, 9])]
    ats = [c[1] for c in lib.calls[n0:] if c[0] in ("mw_snapshot_save_at", "mw_snapshot_save_frames_at")]
    assert [a[3] for a in ats] == [4, 4, 4, 4, 2, 2] and all(a[1] is None and a[2] is not None for a in ats)
    assert (bank.count, bank.capacity, bank.frame_flags, bank.frame_stack) == (10, 10, SNAPF_STACK, 2)
    assert bank.frames is not None and bank.seeds.dtype == torch.int64 and bank.seeds.tolist() == seeds
    # the mode: reset() loads next_level into every env — no world generated, nothing drawn — and step() sits the loads behind the step
    vec.set_levels(bank, generator=torch.Generator().manual_seed(1))
    assert vec.level.dtype == vec.next_level.dtype == torch.int32 and vec.next_level.shape == (4,)
    assert int(vec.next_level.min()) >= 0 and int(vec.next_level.max()) < 10
    chosen = vec.next_level.clone()
    n0 = len(lib.calls)
    assert vec.reset() is vec.obs
    assert _names(lib.calls[n0:]) == ["mw_snapshot_load_where", "mw_snapshot_load_frames_where"]
    load, loadf = [c[1] for c in lib.calls[n0:] if c[0] in NAMES]
    assert load[1].value == loadf[1].value and load[2].value == loadf[2].value == vec.next_level.data_ptr()
    assert load[3].value == bank.data.data_ptr() and load[4:6] == (10, 10)
    assert loadf[4:7] == (10, 10, SNAPF_STACK) and loadf[7].value == vec.obs.data_ptr() and loadf[8] is None
    assert torch.equal(vec.level, chosen)
    n0 = len(lib.calls)
    vec.terminated[2] = 1
    chosen = vec.next_level.clone()
    vec.step(torch.zeros(4, dtype=torch.int32))
    assert _names(lib.calls[n0:]) == ["mw_step", "mw_snapshot_load_where", "mw_snapshot_load_frames_where"]
    assert lib.calls[-1][1][1].value == vec._done.data_ptr() and vec._done.tolist() == [0, 0, 1, 0]
    assert int(vec.level[2]) == int(chosen[2]) and torch.equal(vec.level[:2], vec.played_level[:2])
    n0 = len(lib.calls)
    vec.rollout(torch.zeros((2, 4), dtype=torch.int32), render=False)
    assert _names(lib.calls[n0:]) == ["mw_step_plan", "mw_snapshot_load_where"]


def test_a_snapshot_carries_its_seeds():
    import torch
    from miniworld_amd.vec_env import EnvSnapshot
    data, frames, seeds = torch.arange(64, dtype=torch.uint8), torch.arange(96, dtype=torch.uint8), torch.tensor([7, 9, 11])
    snap = EnvSnapshot(data, 3, 4, frames, SNAPF_STACK, 3, seeds)
    for other in (snap.cpu(), snap.clone(), snap.to("cpu"), EnvSnapshot.from_state_dict(snap.state_dict())):
        assert torch.equal(other.seeds, seeds) and torch.equal(other.data, data) and (other.count, other.capacity) == (3, 4)
    assert snap.clone().seeds.data_ptr() != seeds.data_ptr()
    assert set(snap.state_dict()) == {"data", "count", "capacity", "frames", "frame_flags", "frame_stack", "seeds"}
    # a state dict from before loads, and a snapshot without seeds writes the keys of before
    old = EnvSnapshot.from_state_dict({"data": data, "count": 3, "capacity": 4, "frames": frames, "frame_flags": SNAPF_STACK, "frame_stack": 3})
    assert old.seeds is None and old.clone().seeds is None and "seeds" not in old.state_dict()
