"""Rollout traces (mw_step_plan_trace), host side, without a GPU: the header declares the entry point and its struct, the library
exports it and refuses a call without an engine, and MiniWorldVecEnv.rollout(plans, render, trace, trace_ent) reaches it with a struct
of the data pointers of `vec.trace`'s tensors — or makes exactly the untraced call when no trace is asked for, or raises ValueError
before the library is called.  The recording library is the one of tests/test_rollout_cpu.py."""
import ctypes as C
import os
import re

import pytest

from helpers import stub_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point_and_its_struct():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"typedef struct \{[^}]*double\s*\*agent_pos;[^}]*double\s*\*agent_dir;[^}]*int32_t\s*\*carrying;[^}]*double\s*\*ent_pos;[^}]*"
                     r"int32_t\s+ent_slot;\s*\} mw_plan_trace;", header)
    assert re.search(r"int mw_step_plan_trace\(mw_engine \*e, const int32_t \*d_plans, int32_t horizon, uint8_t \*d_obs, float \*d_depth,\s*"
                     r"float \*d_reward, float \*d_step_reward, uint8_t \*d_term, uint8_t \*d_trunc, int32_t \*d_nsteps,\s*"
                     r"const mw_plan_trace \*trace, void \*stream\);", header)
    assert "miniworld.py:670-730" in header and "entity.py:455-515" in header
    # the ctypes struct is the header's: four pointers, then the slot
    assert [f[0] for f in engine.MwPlanTrace._fields_] == ["agent_pos", "agent_dir", "carrying", "ent_pos", "ent_slot"]
    assert C.sizeof(engine.MwPlanTrace) == 4 * C.sizeof(C.c_void_p) + 8 and engine.MwPlanTrace.ent_slot.offset == 4 * C.sizeof(C.c_void_p)


def test_library_exports_the_entry_point():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    assert hasattr(lib, "mw_step_plan_trace")
    tr = engine.MwPlanTrace()
    assert lib.mw_step_plan_trace(None, None, 2, None, None, None, None, None, None, None, C.byref(tr), None) == -1     # no engine: MW_E_INVALID
    assert lib.mw_step_plan_trace(None, None, 2, None, None, None, None, None, None, None, None, None) == -1
    assert lib.mw_step_plan(None, None, 2, None, None, None, None, None, None, None, None) == -1
    assert lib.mw_abi_version() == 4


def _step_calls(lib):
    return [(name, args) for name, args in lib.calls if name in ("mw_step", "mw_step_repeat", "mw_step_plan", "mw_step_plan_trace")]


def _struct(arg):
    """the MwPlanTrace behind the byref() a traced call passes"""
    from miniworld_amd import engine
    assert isinstance(arg._obj, engine.MwPlanTrace)
    return arg._obj


def test_an_untraced_rollout_is_todays_call(monkeypatch):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, want_depth=True)
    plans = torch.zeros((3, 2), dtype=torch.int32)
    for kw in ({}, {"trace": None}, {"render": False}, {"render": False, "trace": None, "trace_ent": 0}):
        before = len(_step_calls(lib))
        vec.rollout(plans, **kw)
        assert len(_step_calls(lib)) == before + 1
        name, args = _step_calls(lib)[-1]
        assert name == "mw_step_plan" and len(args) == 11 and args[2] == 3
        assert vec.trace is None
    # ... also behind a traced one
    vec.rollout(plans, trace=True)
    assert vec.trace is not None
    vec.rollout(plans)
    assert _step_calls(lib)[-1][0] == "mw_step_plan" and len(_step_calls(lib)[-1][1]) == 11 and vec.trace is None


def test_a_traced_rollout_makes_one_trace_call_with_the_tensors_of_vec_trace(monkeypatch):
    import torch
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, want_depth=True)
    goal = int(vec.engine.cfg.goal_ent)
    plans = torch.zeros((3, 2), dtype=torch.int64)
    out = vec.rollout(plans, trace=True)
    assert len(_step_calls(lib)) == 1
    name, args = _step_calls(lib)[-1]
    assert name == "mw_step_plan_trace" and len(args) == 12 and args[2] == 3
    assert out[0] is vec.obs and args[3].value == vec.obs.data_ptr() and args[4].value == vec.depth.data_ptr()
    assert args[6].value == vec.step_rewards.data_ptr() and args[9].value == vec.substeps.data_ptr()
    t = _struct(args[10])
    assert set(vec.trace) == {"agent_pos", "agent_dir", "carrying"}
    assert tuple(vec.trace["agent_pos"].shape) == (3, 2, 3) and vec.trace["agent_pos"].dtype == torch.float64
    assert tuple(vec.trace["agent_dir"].shape) == (3, 2) and vec.trace["agent_dir"].dtype == torch.float64
    assert tuple(vec.trace["carrying"].shape) == (3, 2) and vec.trace["carrying"].dtype == torch.int32
    assert (t.agent_pos, t.agent_dir, t.carrying) == tuple(vec.trace[k].data_ptr() for k in ("agent_pos", "agent_dir", "carrying"))
    assert not t.ent_pos
    # frameless, with the goal's position: null d_obs / d_depth, the default slot
    out = vec.rollout(plans[:2], render=False, trace=("ent_pos", "agent_pos"))
    name, args = _step_calls(lib)[-1]
    assert len(_step_calls(lib)) == 2 and name == "mw_step_plan_trace" and args[2] == 2 and args[3] is None and args[4] is None and out[0] is None
    t = _struct(args[10])
    assert set(vec.trace) == {"ent_pos", "agent_pos"} and tuple(vec.trace["ent_pos"].shape) == (2, 2, 3)
    assert t.ent_pos == vec.trace["ent_pos"].data_ptr() and t.agent_pos == vec.trace["agent_pos"].data_ptr() and t.ent_slot == goal
    assert not t.agent_dir and not t.carrying
    # a chosen slot
    vec.rollout(plans, render=False, trace=["ent_pos"], trace_ent=0)
    t = _struct(_step_calls(lib)[-1][1][10])
    assert t.ent_slot == 0 and t.ent_pos == vec.trace["ent_pos"].data_ptr() and not t.agent_pos
    # the buffers grow to the largest T seen, and a shorter call reuses them
    vec.rollout(torch.zeros((5, 2), dtype=torch.int32), render=False, trace=True)
    big = vec.trace["agent_pos"].data_ptr()
    assert tuple(vec.trace["agent_pos"].shape) == (5, 2, 3) and _step_calls(lib)[-1][1][2] == 5
    vec.rollout(plans[:2], trace=True)
    assert tuple(vec.trace["agent_pos"].shape) == (2, 2, 3) and vec.trace["agent_pos"].data_ptr() == big
    assert _struct(_step_calls(lib)[-1][1][10]).agent_pos == big


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2)
    E = int(vec.engine.cfg.max_ents)
    plans = torch.zeros((3, 2), dtype=torch.int32)
    before = len(lib.calls)
    for render in (True, False):
        for kw in ({"trace": ("agent_pos", "health")}, {"trace": "agent_pos"}, {"trace": ()}, {"trace": ("ent_pos",), "trace_ent": E},
                   {"trace": ("ent_pos",), "trace_ent": -1}, {"trace": ("ent_pos",), "trace_ent": 0.5}):
            with pytest.raises(ValueError):
                vec.rollout(plans, render=render, **kw)
        for shape in ((2,), (3, 3), (0, 2), (257, 2)):
            with pytest.raises(ValueError):
                vec.rollout(torch.zeros(shape, dtype=torch.int32), render=render, trace=True)
    assert len(lib.calls) == before
    # the engine's own checks: a wrong tensor, no field, a slot out of range
    e = vec.engine
    good = lambda: {"agent_pos": torch.zeros((3, 2, 3), dtype=torch.float64)}
    for trace, slot in (({}, 0), ({"agent_pos": None}, 0), ({"health": torch.zeros((3, 2))}, 0),
                        ({"agent_pos": torch.zeros((3, 2, 3), dtype=torch.float32)}, 0), ({"agent_pos": torch.zeros((2, 2, 3), dtype=torch.float64)}, 0),
                        ({"agent_pos": torch.zeros((3, 3, 3), dtype=torch.float64)}, 0), ({"carrying": torch.zeros((3, 2), dtype=torch.int64)}, 0),
                        ({"agent_dir": torch.zeros((2, 3), dtype=torch.float64).t()}, 0), ({"agent_pos": [0.0]}, 0),
                        ({"ent_pos": torch.zeros((3, 2, 3), dtype=torch.float64)}, E), ({"ent_pos": torch.zeros((3, 2, 3), dtype=torch.float64)}, -1)):
        with pytest.raises(engine.EngineError):
            e.step_plan_trace(plans, None, trace=trace, ent_slot=slot)
    with pytest.raises(engine.EngineError):
        e.step_plan_trace(torch.zeros((3, 3), dtype=torch.int32), None, trace=good())
    assert len(lib.calls) == before
    e.step_plan_trace(plans, None, trace=good(), ent_slot=E + 5)           # (the slot is ent_pos's: not looked at without it)
    assert len(lib.calls) == before + 1
    # CollectHealth: its kits respawn behind the frame
    ch = MiniWorldVecEnv("MiniWorld-CollectHealth-v0", 2)
    before = len(lib.calls)
    with pytest.raises(ValueError):
        ch.rollout(plans, render=False, trace=("agent_pos", "ent_pos"))
    with pytest.raises(engine.EngineError):
        ch.engine.step_plan_trace(plans, None, trace={"ent_pos": torch.zeros((3, 2, 3), dtype=torch.float64)})
    assert len(lib.calls) == before
    ch.rollout(plans, render=False, trace=True)
    assert lib.calls[-1][0] == "mw_step_plan_trace"
    # seed mode: a frameless call is refused with a trace as without
    monkeypatch.setattr(vec, "next_seed", torch.zeros(2, dtype=torch.int64), raising=False)
    before = len(lib.calls)
    with pytest.raises(ValueError):
        vec.rollout(plans, render=False, trace=True)
    assert len(lib.calls) == before


def test_the_committed_resource_usage_lists_the_trace_kernels_as_new():
    """profiles/r19/resource_usage.txt is tools/perf/resource_usage.py's output over the parent commit's and this tree's compile logs:
    every kernel of the parent unchanged, the four trace kernels new."""
    text = open(os.path.join(ROOT, "profiles", "r19", "resource_usage.txt")).read()
    assert re.search(r"^differing kernels: 0 of 94$", text, re.M)
    new = text.split("# kernels only this tree has")[1]
    names = re.findall(r"^(\w+) \| - \|", new, re.M)
    assert sorted(names) == sorted("mw_step_trace" + s + "_kernel" for s in ("", "_pcg", "_dense", "_dense_pcg")), names
