"""Frame stacking (mw_set_frame_stack), host side, without a GPU: the header declares the entry points and constants, the ABI version
did not move, the library exports them, the ring rule engine.stack_slots states is right for every depth, and
MiniWorldVecEnv(frame_stack=) / MiniWorldVectorEnv(frame_stack=) validate their arguments before an engine exists, reach the
entry points with the buffers they should and report the stacked shapes."""
import os
import re

import numpy as np
import pytest

from helpers import stub_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_set_frame_stack\(mw_engine \*e, int32_t depth, int32_t pad, uint8_t \*d_ring, uint8_t \*d_final_stack[^)]*\);", header)
    assert re.search(r"#define MW_MAX_STACK 16\b", header) and engine.MAX_STACK == 16
    assert re.search(r"enum \{ MW_STACK_PAD_RESET = 0, MW_STACK_PAD_ZERO = 1 \};", header)
    assert (engine.STACK_PAD_RESET, engine.STACK_PAD_ZERO) == (0, 1)
    # the comments name what the entry points replace
    assert "FrameStackObservation" in header and "VecFrameStack" in header


def test_library_exports_the_entry_points():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    for name in ("mw_set_frame_stack", "mw_stack_refresh", "mw_stack_window"):
        assert hasattr(lib, name), name
    assert lib.mw_set_frame_stack(None, 4, 0, None, None) == -1         # no engine: MW_E_INVALID
    assert lib.mw_stack_refresh(None, None, None) == -1
    assert lib.mw_stack_window(None, None, None) == -1
    assert lib.mw_abi_version() == 4


@pytest.mark.parametrize("K", range(2, 17))
def test_stack_slots_against_a_simulated_ring(K):
    """A ring of 2K - 1 slots written by the rule for 5K pushes: the window after push j holds the last K pushed frames in order
    (as far as that many exist: the engine never shows such a window, a rebuild fills every slot first), and from push K - 1
    on no window reads a slot that was never written."""
    from miniworld_amd.engine import stack_slots
    ring = np.full(2 * K - 1, -1, np.int64)         # the frame number each slot holds; -1 = never written
    for j in range(5 * K):
        writes, first = stack_slots(K, j)
        assert 1 <= len(writes) <= 2 and len(set(writes)) == len(writes) and all(0 <= s < 2 * K - 1 for s in writes)
        assert writes[0] == j % K + K - 1 and (len(writes) == 2) == (j % K >= 1) and first == j % K
        ring[list(writes)] = j
        window = ring[first:first + K]
        assert len(window) == K
        have = min(j + 1, K)
        assert np.array_equal(window[K - have:], np.arange(j + 1 - have, j + 1)), (K, j, window)
        if j >= K - 1:
            assert (window >= 0).all()
        else:       # the slots older than the first push: never written, never a later frame
            assert (window[:K - have] == -1).all(), (K, j, window)


def test_a_rebuild_shows_the_pad_leaving_one_frame_at_a_time():
    """What the push kernel's rebuild relies on: with the frame in the two slots a push of phase p writes and the pad in every
    other slot, the windows of the following ordinary pushes are pad x (K - 1 - t), frame, new frames."""
    from miniworld_amd.engine import stack_slots
    for K in range(2, 17):
        for j0 in range(K):
            ring = np.full(2 * K - 1, -7, np.int64)         # -7: the pad
            ring[list(stack_slots(K, j0)[0])] = 0           # the rebuild's frame
            for t in range(1, K + 2):
                writes, first = stack_slots(K, j0 + t)
                ring[list(writes)] = t
                want = np.array(([-7] * K + list(range(t + 1)))[-K:])
                assert np.array_equal(ring[first:first + K], want), (K, j0, t)


@pytest.mark.parametrize("kw", [dict(frame_stack=1), dict(frame_stack=0), dict(frame_stack=17), dict(frame_stack=-2), dict(frame_stack=2.0),
                                dict(frame_stack=4, stack_pad="edge"), dict(frame_stack=4, stack_pad=0)])
def test_bad_arguments_raise_before_any_engine_exists(kw, monkeypatch):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    from miniworld_amd.vector import MiniWorldVectorEnv
    lib = stub_engine(monkeypatch)
    made = lib.engines
    for cls in (MiniWorldVecEnv, MiniWorldVectorEnv):
        with pytest.raises(ValueError):
            cls("MiniWorld-Hallway-v0", 2, **kw)
    assert made == [] and lib.calls == []


def test_vec_env_reaches_the_entry_points(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch)
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 3, frame_stack=4, stack_pad="zero", final_obs=True)
    (name, args), = [c for c in lib.calls if c[0] == "mw_set_frame_stack"]
    assert args[1:3] == (4, engine.STACK_PAD_ZERO)
    assert tuple(vec._ring.shape) == (3, 7, 60, 80, 3) and vec._ring.dtype == torch.uint8 and args[3].value == vec._ring.data_ptr()
    assert tuple(vec.final_stack.shape) == (3, 4, 60, 80, 3) and args[4].value == vec.final_stack.data_ptr()
    # the stack is set under the env's layout, behind mw_set_obs_layout and mw_set_final_obs
    order = [c[0] for c in lib.calls]
    assert order.index("mw_set_obs_layout") < order.index("mw_set_final_obs") < order.index("mw_set_frame_stack")
    vec.reset()
    assert [c[0] for c in lib.calls][-3:] == ["mw_reset", "mw_render", "mw_stack_refresh"]
    assert lib.calls[-1][1][1].value == vec.obs.data_ptr()
    out = vec.step(torch.zeros(3, dtype=torch.int32))
    assert len(out) == 4 and out[0] is vec.obs                  # what step() returns did not change
    st = vec.stack
    assert tuple(st.shape) == (3, 4, 60, 80, 3) and st.untyped_storage().data_ptr() == vec._ring.untyped_storage().data_ptr()
    plain = MiniWorldVecEnv("MiniWorld-Hallway-v0", 3)
    assert plain.frame_stack is None and plain.stack is None and plain.final_stack is None
    assert sum(c[0] == "mw_set_frame_stack" for c in lib.calls) == 1


@pytest.mark.parametrize("layout, frame, dtype", [("hwc", (60, 80, 3), np.uint8), ("cwh", (3, 80, 60), np.uint8), ("grey", (60, 80, 1), np.float64)])
def test_vector_env_adapter_reports_the_stacked_spaces(layout, frame, dtype, monkeypatch):
    from miniworld_amd import engine
    from miniworld_amd.vector import MiniWorldVectorEnv
    lib = stub_engine(monkeypatch)
    made = lib.engines
    # (the stub's constructor knows no layout: follow mw_set_obs_layout like the real one does)
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, frame_stack=3, obs_layout=layout)
    assert made[0].obs_layout == {"hwc": engine.OBS_HWC_U8, "cwh": engine.OBS_CWH_U8, "grey": engine.OBS_GREY_F64}[layout]
    assert envs.single_observation_space.shape == (3,) + frame and envs.single_observation_space.dtype == dtype
    assert envs.observation_space.shape == (2, 3) + frame
    obs, info = envs.reset(seed=0)
    assert tuple(obs.shape) == (2, 3) + frame and info == {}
    obs = envs.step(np.zeros(2, np.int64))[0]
    assert tuple(obs.shape) == (2, 3) + frame
    host = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, frame_stack=2, to_numpy=True, final_obs=True)
    obs, _, _, _, info = host.step(np.zeros(2, np.int64))
    assert isinstance(obs, np.ndarray) and obs.shape == (2, 2, 60, 80, 3)
    assert info["final_obs"].shape == (2, 2, 60, 80, 3)
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2)
    assert plain.single_observation_space.shape == (60, 80, 3)
