"""Final observations of the same-step auto-reset (mw_set_final_obs), host side, without a GPU: the header declares the entry
point, the library exports it, the ABI version did not move, and the Python layers refuse the flag outside same-step before
anything touches the device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_mw_set_final_obs():
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_set_final_obs\(mw_engine \*e, uint8_t \*d_final_obs, float \*d_final_depth\);", header)


def test_library_exports_mw_set_final_obs():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    assert hasattr(lib, "mw_set_final_obs")
    assert lib.mw_set_final_obs(None, None, None) == -1       # no engine: MW_E_INVALID


@pytest.mark.parametrize("mode", ["next_step", False])
def test_vec_env_rejects_final_obs_outside_same_step(mode):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    with pytest.raises(ValueError, match="final_obs"):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, autoreset=mode, final_obs=True)


def test_vector_env_rejects_final_obs_in_next_step_mode():
    from miniworld_amd.vector import MiniWorldVectorEnv
    with pytest.raises(ValueError, match="final_obs"):
        MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, autoreset_mode="next-step", final_obs=True)
