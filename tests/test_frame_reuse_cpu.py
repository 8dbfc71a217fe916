"""Frame reuse (mw_set_frame_reuse / mw_get_frame_clean), host side, without a GPU: the header declares both entry points, the
ABI version did not move, the library exports them, and MiniWorldVecEnv's switch and MW_FRAME_REUSE=0 reach mw_set_frame_reuse."""
import os
import re

import pytest

from helpers import stub_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points():
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_set_frame_reuse\(mw_engine \*e, int32_t on\);", header)
    assert re.search(r"int mw_get_frame_clean\(mw_engine \*e, uint8_t \*d_out, void \*stream\);", header)


def test_library_exports_the_entry_points():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    assert hasattr(lib, "mw_set_frame_reuse") and hasattr(lib, "mw_get_frame_clean")
    assert lib.mw_set_frame_reuse(None, 1) == -1 and lib.mw_get_frame_clean(None, None, None) == -1      # no engine: MW_E_INVALID
    assert lib.mw_abi_version() == 4


def _reuse_calls(lib):
    return [int(args[1]) for name, args in lib.calls if name == "mw_set_frame_reuse"]


@pytest.mark.parametrize("kwargs,env,want", [
    ({}, None, 1),                              # the env owns its tensors: on by default
    ({"frame_reuse": True}, None, 1),
    ({"frame_reuse": False}, None, 0),          # the constructor's switch
    ({}, "0", 0),                               # MW_FRAME_REUSE=0 forces it off ...
    ({"frame_reuse": True}, "0", 0),            # ... whatever the caller asks for
    ({}, "1", 1),
])
def test_vec_env_switch_and_environment_reach_the_engine(kwargs, env, want, monkeypatch):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    if env is None:
        monkeypatch.delenv("MW_FRAME_REUSE", raising=False)
    else:
        monkeypatch.setenv("MW_FRAME_REUSE", env)
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, **kwargs)
    assert _reuse_calls(lib) == [want]
    assert vec.frame_reuse == bool(want) and vec.engine.frame_reuse == bool(want)


def test_engine_reports_what_is_in_effect(monkeypatch):
    from miniworld_amd import engine
    from miniworld_amd.scene import base_config
    lib = stub_engine(monkeypatch)
    e = engine.Engine(base_config(4, 80, 60, 1, 6, 4, 16))
    monkeypatch.delenv("MW_FRAME_REUSE", raising=False)
    assert e.set_frame_reuse(True) is True and e.set_frame_reuse(False) is False
    monkeypatch.setenv("MW_FRAME_REUSE", "0")
    assert e.set_frame_reuse(True) is False
    assert _reuse_calls(lib) == [1, 0, 0]
