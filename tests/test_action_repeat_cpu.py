"""Action repeat (mw_step_repeat), host side, without a GPU: the header declares the entry point and its cap, the ABI version did
not move, the library exports it, and MiniWorldVecEnv.step(actions, repeat) / MiniWorldVectorEnv(action_repeat=) reach it — or
mw_step, for a repeat of 1 — with the arguments they should."""
import os
import re

import numpy as np
import pytest

from helpers import stub_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_step_repeat\(mw_engine \*e, const int32_t \*d_actions, int32_t repeat, uint8_t \*d_obs, float \*d_depth,\s*"
                     r"float \*d_reward, uint8_t \*d_term, uint8_t \*d_trunc, int32_t \*d_nsteps, void \*stream\);", header)
    assert re.search(r"#define MW_MAX_REPEAT 256\b", header) and engine.MAX_REPEAT == 256


def test_library_exports_the_entry_point():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    assert hasattr(lib, "mw_step_repeat")
    assert lib.mw_step_repeat(None, None, 2, None, None, None, None, None, None, None) == -1        # no engine: MW_E_INVALID
    assert lib.mw_abi_version() == 4


def _step_calls(lib):
    return [(name, args) for name, args in lib.calls if name in ("mw_step", "mw_step_repeat")]


def test_vec_env_step_picks_the_entry_point(monkeypatch):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2)
    a = torch.zeros(2, dtype=torch.int32)
    vec.step(a)
    vec.step(a, repeat=1)
    assert [name for name, _ in _step_calls(lib)] == ["mw_step", "mw_step"] and vec.substeps is None
    out = vec.step(a, repeat=3)
    assert len(out) == 4
    name, args = _step_calls(lib)[-1]
    assert name == "mw_step_repeat" and len(args) == 10 and args[2] == 3
    assert vec.substeps is not None and vec.substeps.dtype == torch.int32 and tuple(vec.substeps.shape) == (2,)
    assert args[8] is not None and args[8].value == vec.substeps.data_ptr()         # d_nsteps
    assert args[3].value == vec.obs.data_ptr() and args[5].value == vec.reward.data_ptr()


@pytest.mark.parametrize("repeat", [0, -1, 257])
def test_a_repeat_out_of_range_raises_before_any_library_call(repeat, monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2)
    before = len(lib.calls)
    with pytest.raises(engine.EngineError):
        vec.step(torch.zeros(2, dtype=torch.int32), repeat=repeat)
    assert len(lib.calls) == before


def test_vector_env_adapter_reports_substeps(monkeypatch):
    from miniworld_amd.vector import MiniWorldVectorEnv
    lib = stub_engine(monkeypatch)
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, action_repeat=3)
    info = envs.step(np.zeros(2, np.int64))[4]
    name, args = _step_calls(lib)[-1]
    assert name == "mw_step_repeat" and args[2] == 3
    assert "substeps" in info and tuple(info["substeps"].shape) == (2,)
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2)
    info = plain.step(np.zeros(2, np.int64))[4]
    assert _step_calls(lib)[-1][0] == "mw_step" and set(info) == {"_final_info"}
    with pytest.raises(ValueError):
        MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, action_repeat=0)
