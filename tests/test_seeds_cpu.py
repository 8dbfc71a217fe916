"""Seeded resets on the device (mw_reset_where, mw_set_reset_seeds), host side, without a GPU: the seeding arithmetic the host and the
kernels share (miniworld_amd/csrc/mw_rng.h: mw::pcg64_seed) against numpy for edge and random 64-bit seeds, through mw_pcg64_draws; the
header, the export list and the null-engine refusals; the launch policy's decisions for the mode (mw_policy.h, compiled for the host
from tests/hostcheck/seeds_policy.cpp); and MiniWorldVecEnv's autoreset="seeds" bookkeeping over a stub engine."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from test_launch_policy_cpu import policy_lib
from helpers import stub_engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "seeds_policy.cpp")
LIB = os.path.join(HERE, "hostcheck", "libmwseeds.so")
NAMES = ("mw_reset_where", "mw_set_reset_seeds")
EDGE_SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 + 5, 2 ** 64 - 1]
CALL_RENDER, CALL_STEP, CALL_TERMINAL_STEP, CALL_LIST_PASS = 0, 1, 2, 3
STEP_REFUSED, STEP_FRAMELESS, STEP_ONE_PASS, STEP_TWO_PASS = -1, 0, 1, 2
PATH_TILE, PATH_QUAD = 0, 1
TASK_COLLECT = 6


def _ask(what, args, n):
    lib = policy_lib(SRC, LIB)
    a, out = np.array(list(args) + [0], np.int64), np.zeros(8, np.int64)
    assert lib.mwpol(what, a.ctypes.data, out.ctypes.data) == n
    return out[:n].tolist()


# ---------------------------------------------------------------------------------------------------------------- seeding

def test_the_shared_seeding_is_numpys_for_edge_and_random_seeds():
    """mw_pcg64_draws seeds through mw::pcg64_seed, the function the kernels seed with: SeedSequence(s).generate_state(4, uint64) and
    pcg_setseq_128_srandom_r, one entropy word below 2^32 and two from there on.  The first draws of Generator(PCG64(SeedSequence(s)))
    depend on every bit of state and increment."""
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    rng = np.random.default_rng(20261018)
    seeds = EDGE_SEEDS + [int(s) for s in rng.integers(0, 2 ** 64, 300, dtype=np.uint64)] + [int(s) for s in rng.integers(0, 2 ** 32, 40, dtype=np.uint64)]
    for seed in seeds:
        out = np.zeros(8)
        assert lib.mw_pcg64_draws(C.c_uint64(seed), 8, None, out.ctypes.data) == 0
        want = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed))).random(8)
        assert np.array_equal(out, want), seed


def test_one_statement_of_the_seeding_arithmetic():
    """The SeedSequence constants live in mw_rng.h alone; mw_assets.h and the host runtime call it."""
    csrc = os.path.join(ROOT, "miniworld_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip")) and "0x43b0d7e5" in open(os.path.join(csrc, f)).read()]
    assert holders == ["mw_rng.h"]
    assert "mw::pcg64_seed(seed, out)" in open(os.path.join(csrc, "mw_assets.h")).read()
    host = open(os.path.join(csrc, "mw_engine.hip")).read()
    assert "mw::rng_seed_words(" in host and "mwasset::pcg64_seed(seed, s)" in host


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_header_declares_the_entry_points():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_set_reset_seeds\(mw_engine \*e, const uint64_t \*d_next_seed /\* \[N\], device; NULL = off \*/\);", header)
    text = " ".join(header.split())
    assert "miniworld.py:544-604" in text and "scripts/benchmark.py:36-37" in text
    assert "FRAMELESS mw_step_plan (d_obs == NULL) is MW_E_INVALID" in text


def test_library_exports_the_entry_points_and_refuses_a_null_engine():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    mask, seeds = (C.c_uint8 * 4)(1, 1, 1, 1), (C.c_uint64 * 4)(1, 2, 3, 4)
    m, s = C.cast(mask, C.c_void_p), C.cast(seeds, C.c_void_p)
    assert lib.mw_reset_where(None, m, s, None) == -1       # no engine: MW_E_INVALID
    assert lib.mw_set_reset_seeds(None, s) == -1
    assert lib.mw_set_reset_seeds(None, None) == -1


# ---------------------------------------------------------------------------------------------------------------- the policy

@pytest.mark.parametrize("seeds,final,frameless", list(itertools.product((0, 1), repeat=3)))
def test_the_passes_of_a_step_call(seeds, final, frameless):
    """Seeds on or off x final buffers on or off x drawn or frameless."""
    shape, final_copy, seeded_install = _ask(0, [seeds, final, frameless], 3)
    if frameless:
        assert (shape, final_copy, seeded_install) == (STEP_REFUSED if seeds else STEP_FRAMELESS, 0, 0)
    elif not seeds and not final:
        assert (shape, final_copy, seeded_install) == (STEP_ONE_PASS, 0, 0)
    else:
        assert (shape, final_copy, seeded_install) == (STEP_TWO_PASS, final, seeds)


def test_the_frame_policy_of_a_seeded_steps_passes():
    """Without seeds the passes of a two-pass step draw every env and hold nothing, as before.  With seeds the first pass is a plain
    step to frame reuse and the frame cache, the list pass is not, and both leave the call's buffers held."""
    def pol(kind, seeded, path=PATH_QUAD, task=0, view=0, held=1):
        return _ask(1, [kind, view, 1, held, 0, 0, 0, task, 1, path, seeded], 4)
    step = pol(CALL_STEP, 0)
    assert step == [1, 1, 1, 1]
    assert pol(CALL_STEP, 1) == step and pol(CALL_RENDER, 1) == pol(CALL_RENDER, 0) == [0, 0, 0, 1]
    assert pol(CALL_TERMINAL_STEP, 0) == [0, 0, 0, 0] and pol(CALL_LIST_PASS, 0) == [0, 0, 0, 0]
    assert pol(CALL_TERMINAL_STEP, 1) == step
    assert pol(CALL_LIST_PASS, 1) == [0, 0, 0, 1]
    assert pol(CALL_TERMINAL_STEP, 1, held=0) == [0, 1, 1, 1]
    assert pol(CALL_TERMINAL_STEP, 1, path=PATH_TILE) == [1, 0, 0, 1]
    assert pol(CALL_TERMINAL_STEP, 1, task=TASK_COLLECT) == [1, 1, 0, 1]
    assert pol(CALL_TERMINAL_STEP, 1, view=1) == [0, 0, 0, 0]


def test_what_a_masked_seeded_reset_invalidates():
    """The held frame goes; the other envs' cached frames stay (the kernel advances the epochs of the envs it writes)."""
    assert _ask(2, [], 2) == [1, 0]


# ---------------------------------------------------------------------------------------------------------------- the vec env

def _names(calls):
    return [c[0] for c in calls]


def test_seed_mode_bookkeeping_over_a_stub_engine(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    resets = []
    monkeypatch.setattr(engine.Engine, "reset", lambda self, mask=None, seeds=None: (lib.calls.append(("mw_reset", ())), resets.append((mask, seeds.copy())))[0])
    n0 = len(lib.calls)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, autoreset="seeds", final_obs=True)
    assert vec.autoreset_mode == "seeds" and vec.engine.cfg.autoreset == 1        # MW_AUTORESET_SAME_STEP
    assert vec.next_seed.dtype == vec.episode_seed.dtype == torch.int64 and vec.next_seed.shape == (4,)
    sets = [c for c in lib.calls[n0:] if c[0] == "mw_set_reset_seeds"]
    assert len(sets) == 1 and sets[0][1][1].value == vec.next_seed.data_ptr()
    vec.reset(seed=100)
    assert resets[-1][0] is None and resets[-1][1].tolist() == [100, 101, 102, 103]
    assert vec.episode_seed.tolist() == [100, 101, 102, 103] and vec.next_seed.tolist() == [104, 105, 106, 107]
    # a step that ends envs 1 and 3: episode_seed follows, their next_seed moves N on; the caller's write in between wins
    vec.next_seed[3] = 9000
    vec.terminated[1], vec.truncated[3] = 1, 1
    n0 = len(lib.calls)
    vec.step(torch.zeros(4, dtype=torch.int32))
    assert _names(lib.calls[n0:]) == ["mw_step"]
    assert vec.episode_seed.tolist() == [100, 105, 102, 9000] and vec.next_seed.tolist() == [104, 109, 106, 9004]
    vec.terminated.zero_()
    vec.truncated.zero_()
    vec.rollout(torch.zeros((2, 4), dtype=torch.int32))
    assert vec.episode_seed.tolist() == [100, 105, 102, 9000]
    n0 = len(lib.calls)
    with pytest.raises(ValueError, match="frameless"):
        vec.rollout(torch.zeros((2, 4), dtype=torch.int32), render=False)
    with pytest.raises(ValueError, match="seed"):
        vec.reset(seed=-1)
    with pytest.raises(ValueError, match="non-negative"):
        vec.reset_where([1, 0, 0, 0], [-5, 0, 0, 0])
    assert lib.calls[n0:] == []
    # reset_where: the binding, then the reset path's frame; episode_seed follows the mask
    n0 = len(lib.calls)
    assert vec.reset_where([0, 1, 1, 0], [7, 2 ** 63 + 5, 11, 13]) is vec.obs
    assert _names(lib.calls[n0:]) == ["mw_reset_where", "mw_render"]
    assert vec.episode_seed.tolist() == [100, (2 ** 63 + 5) - 2 ** 64, 11, 9000]
    with pytest.raises(ValueError):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, autoreset="seed")
    plain = MiniWorldVecEnv("MiniWorld-Hallway-v0", 4)
    assert plain.next_seed is None and plain.episode_seed is None


def test_the_adapter_reports_the_played_seed(monkeypatch):
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 3, reset_seeds=[50, 60, 70])
    assert envs.vec.autoreset_mode == "seeds"
    envs.reset(seed=5)
    assert envs.vec.episode_seed.tolist() == [5, 6, 7] and envs.vec.next_seed.tolist() == [50, 60, 70]
    envs.vec.terminated[2] = 1
    *_, info = envs.step(torch.zeros(3, dtype=torch.int32))
    assert info["seed"].tolist() == [5, 6, 7] and info["_final_info"].tolist() == [False, False, True]
    assert envs.vec.episode_seed.tolist() == [5, 6, 70] and envs.vec.next_seed.tolist() == [50, 60, 73]
    for bad in (dict(levels=[1, 2]), dict(autoreset_mode="next-step"), dict(autoreset=False)):
        with pytest.raises(ValueError):
            MiniWorldVectorEnv("MiniWorld-Hallway-v0", 3, reset_seeds=True, **bad)
    with pytest.raises(ValueError):
        MiniWorldVectorEnv("MiniWorld-Hallway-v0", 3, reset_seeds=[1, -2, 3])
