"""The frame cache (mw_set_frame_cache / mw_get_frame_source), host side, without a GPU: the header declares both entry points, the
ABI version did not move, the library exports them, and MiniWorldVecEnv's keyword, the vector adapter's and MW_FRAME_CACHE=0 reach
mw_set_frame_cache."""
import os
import re

import pytest

from helpers import stub_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points():
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_set_frame_cache\(mw_engine \*e, int32_t slots\);", header)
    assert re.search(r"int mw_get_frame_source\(mw_engine \*e, uint8_t \*d_out, void \*stream\);", header)


def test_library_exports_the_entry_points():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    assert hasattr(lib, "mw_set_frame_cache") and hasattr(lib, "mw_get_frame_source")
    assert lib.mw_set_frame_cache(None, 4) == -1 and lib.mw_get_frame_source(None, None, None) == -1      # no engine: MW_E_INVALID
    assert lib.mw_abi_version() == 4


def _cache_calls(lib):
    return [int(args[1]) for name, args in lib.calls if name == "mw_set_frame_cache"]


def _environment(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("MW_FRAME_CACHE", raising=False)
    else:
        monkeypatch.setenv("MW_FRAME_CACHE", value)


CASES = [
    ({}, None, 4),                              # four slots by default
    ({"frame_cache": 8}, None, 8),
    ({"frame_cache": 2}, None, 2),
    ({"frame_cache": 0}, None, 0),              # the constructor's switch
    ({}, "0", 0),                               # MW_FRAME_CACHE=0 forces it off ...
    ({"frame_cache": 8}, "0", 0),               # ... whatever the caller asks for
    ({}, "1", 4),
]


@pytest.mark.parametrize("kwargs,env,want", CASES)
def test_vec_env_keyword_and_environment_reach_the_engine(kwargs, env, want, monkeypatch):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _environment(monkeypatch, env)
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, **kwargs)
    assert _cache_calls(lib) == [want]
    assert vec.frame_cache == want and vec.engine.frame_cache == want


@pytest.mark.parametrize("kwargs,env,want", CASES)
def test_vector_adapter_passes_the_keyword_on(kwargs, env, want, monkeypatch):
    from miniworld_amd.vector import MiniWorldVectorEnv
    _environment(monkeypatch, env)
    lib = stub_engine(monkeypatch)
    venv = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, **kwargs)
    assert _cache_calls(lib) == [want] and venv.vec.frame_cache == want


@pytest.mark.parametrize("bad", [-1, 9, 2.0, True, "4", None])
def test_slot_counts_outside_the_range_are_refused(bad, monkeypatch):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    _environment(monkeypatch, None)
    lib = stub_engine(monkeypatch)
    with pytest.raises(ValueError):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, frame_cache=bad)
    assert _cache_calls(lib) == []


def test_engine_reports_what_is_in_effect(monkeypatch):
    from miniworld_amd import engine
    from miniworld_amd.scene import base_config
    lib = stub_engine(monkeypatch)
    e = engine.Engine(base_config(4, 80, 60, 1, 6, 4, 16))
    _environment(monkeypatch, None)
    assert e.set_frame_cache(4) == 4 and e.set_frame_cache(0) == 0
    _environment(monkeypatch, "0")
    assert e.set_frame_cache(4) == 0 and e.frame_cache == 0
    assert _cache_calls(lib) == [4, 0, 0]
