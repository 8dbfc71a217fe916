"""Open-loop rollouts (mw_step_plan), host side, without a GPU: the header declares the entry point and its cap, the library
exports it and refuses a call without an engine, and MiniWorldVecEnv.rollout(plans, render) reaches it with the arguments it
should — a null d_obs / d_depth for the frameless call — or raises ValueError before the library is called."""
import os
import re

import pytest

from helpers import stub_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_step_plan\(mw_engine \*e, const int32_t \*d_plans /\* \[horizon\]\[N\] \*/, int32_t horizon,\s*"
                     r"uint8_t \*d_obs, float \*d_depth, float \*d_reward, float \*d_step_reward /\* \[horizon\]\[N\] or NULL \*/,\s*"
                     r"uint8_t \*d_term, uint8_t \*d_trunc, int32_t \*d_nsteps, void \*stream\);", header)
    assert re.search(r"#define MW_MAX_PLAN MW_MAX_REPEAT\b", header) and engine.MAX_PLAN == engine.MAX_REPEAT == 256


def test_library_exports_the_entry_point():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    assert hasattr(lib, "mw_step_plan")
    assert lib.mw_step_plan(None, None, 2, None, None, None, None, None, None, None, None) == -1        # no engine: MW_E_INVALID
    assert lib.mw_abi_version() == 4


def _step_calls(lib):
    return [(name, args) for name, args in lib.calls if name in ("mw_step", "mw_step_repeat", "mw_step_plan")]


def test_rollout_makes_one_plan_call_drawn_or_frameless(monkeypatch):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, want_depth=True)
    plans = torch.zeros((3, 2), dtype=torch.int64)          # (int64, as torch.randint gives: converted)
    out = vec.rollout(plans)
    assert len(_step_calls(lib)) == 1
    name, args = _step_calls(lib)[-1]
    assert name == "mw_step_plan" and len(args) == 11 and args[2] == 3
    assert out[0] is vec.obs and out[1] is vec.reward and out[2] is vec.terminated and out[3] is vec.truncated
    assert args[3].value == vec.obs.data_ptr() and args[4].value == vec.depth.data_ptr() and args[5].value == vec.reward.data_ptr()
    assert vec.substeps is not None and vec.substeps.dtype == torch.int32 and args[9].value == vec.substeps.data_ptr()
    assert vec.step_rewards.dtype == torch.float32 and tuple(vec.step_rewards.shape) == (3, 2)
    assert args[6].value == vec.step_rewards.data_ptr()
    out = vec.rollout(plans[:2].to(torch.int32), render=False)
    assert len(_step_calls(lib)) == 2
    name, args = _step_calls(lib)[-1]
    assert name == "mw_step_plan" and args[2] == 2 and args[3] is None and args[4] is None      # null d_obs / d_depth
    assert out[0] is None and out[1] is vec.reward
    assert tuple(vec.step_rewards.shape) == (2, 2) and args[6].value == vec.step_rewards.data_ptr()
    vec.rollout(torch.zeros((5, 2), dtype=torch.int32), render=False)       # the buffer grows to the largest T seen
    assert tuple(vec.step_rewards.shape) == (5, 2) and _step_calls(lib)[-1][1][2] == 5


@pytest.mark.parametrize("shape", [(2,), (3, 2, 1), (3, 3), (0, 2), (257, 2)])
def test_a_wrong_plan_shape_raises_before_any_library_call(shape, monkeypatch):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2)
    before = len(lib.calls)
    for render in (True, False):
        with pytest.raises(ValueError):
            vec.rollout(torch.zeros(shape, dtype=torch.int32), render=render)
    assert len(lib.calls) == before
