"""The binding hands raw addresses to kernels, so a tensor of the wrong dtype, size or stride pattern must never reach the library.  Over
the stub engine (helpers.stub_engine), CPU tensors: for every tensor argument of a public Engine method that is checked rather than
converted, a wrong dtype, a wrong element count and a non-contiguous tensor each raise EngineError before any entry point is called
(mw_snapshot_bytes / mw_snapshot_frames_bytes, the size queries a record buffer is measured against, launch nothing and do not count).
Not in the table: `actions`, `plans` and the index arrays of the snapshot calls, which are converted (their count is checked below),
and render / render_top / stack_refresh, whose buffers the caller lays out (render_top_view switches the layout around its call)."""
import pytest
import torch

from helpers import stub_engine

N, E, H, W, T, R, K = 4, 2, 60, 80, 3, 5, 2
GX, GZ = 6, 3
U8, I32, I64, F32, F64, U16 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64, torch.uint16
OTHER = {U8: torch.int8, I32: I64, I64: I32, F32: F64, F64: F32, U16: torch.int16}
SIZE_QUERIES = {"mw_snapshot_bytes", "mw_snapshot_frames_bytes"}


def make(dtype, shape):
    if dtype is U16:        # (few CPU kernels of its own: made as int16)
        return torch.zeros(shape, dtype=torch.int16).view(U16)
    return torch.zeros(shape, dtype=dtype)


def obs():
    return make(U8, (N, H, W, 3))


def depth():
    return make(F32, (N, H, W, 1))


def acts():
    return make(I32, (N,))


def plans():
    return make(I32, (T, N))


def buf():
    return make(U8, (4096,))


def mask():
    return make(U8, (N,))


def recs():
    return make(I32, (N,))


def nav(eng):
    return eng.MwNavParams(0.5, 0.25, 0.0, GX, GZ, 0, 0)


def field():
    return make(U16, (N, GZ, GX))


def ray(eng):
    return eng.MwRayParams(1.0, 0.0, R, 0)


def t_out():
    return make(F64, (N, R))


# (label, dtype, shape, call(engine, engine module, the tensor under test))
TABLE = [
    ("step obs", U8, (N, H, W, 3), lambda e, m, t: e.step(acts(), t)),
    ("step depth", F32, (N, H, W, 1), lambda e, m, t: e.step(acts(), obs(), t)),
    ("step reward", F32, (N,), lambda e, m, t: e.step(acts(), obs(), reward=t)),
    ("step term", U8, (N,), lambda e, m, t: e.step(acts(), obs(), term=t)),
    ("step trunc", U8, (N,), lambda e, m, t: e.step(acts(), obs(), trunc=t)),
    ("step_repeat obs", U8, (N, H, W, 3), lambda e, m, t: e.step_repeat(acts(), 2, t)),
    ("step_repeat nsteps", I32, (N,), lambda e, m, t: e.step_repeat(acts(), 2, obs(), nsteps=t)),
    ("step_plan obs", U8, (N, H, W, 3), lambda e, m, t: e.step_plan(plans(), t)),
    ("step_plan step_reward", F32, (T, N), lambda e, m, t: e.step_plan(plans(), obs(), step_reward=t)),
    ("step_plan nsteps", I32, (N,), lambda e, m, t: e.step_plan(plans(), obs(), nsteps=t)),
    ("step_plan_trace agent_pos", F64, (T, N, 3), lambda e, m, t: e.step_plan_trace(plans(), obs(), trace={"agent_pos": t})),
    ("step_plan_trace carrying", I32, (T, N), lambda e, m, t: e.step_plan_trace(plans(), obs(), trace={"carrying": t})),
    ("set_final_obs obs", U8, (N, H, W, 3), lambda e, m, t: e.set_final_obs(t)),
    ("set_final_obs depth", F32, (N, H, W, 1), lambda e, m, t: e.set_final_obs(obs(), t)),
    ("set_frame_stack ring", U8, (N, 2 * K - 1, H, W, 3), lambda e, m, t: e.set_frame_stack(K, 0, t)),
    ("set_frame_stack final_stack", U8, (N, K, H, W, 3), lambda e, m, t: e.set_frame_stack(K, 0, make(U8, (N, 2 * K - 1, H, W, 3)), t)),
    ("get_state_device agent_pos", F64, (N, 3), lambda e, m, t: e.get_state_device({"agent_pos": t})),
    ("get_state_device ent_kind", I32, (N, E), lambda e, m, t: e.get_state_device({"ent_kind": t})),
    ("set_state_where mask", U8, (N,), lambda e, m, t: e.set_state_where(t, {"agent_dir": make(F64, (N,))})),
    ("set_state_where ent_pos", F64, (N, E, 3), lambda e, m, t: e.set_state_where(mask(), {"ent_pos": t})),
    ("nav_build field", U16, (N, GZ, GX), lambda e, m, t: e.nav_build(nav(m), t)),
    ("nav_build mask", U8, (N,), lambda e, m, t: e.nav_build(nav(m), field(), t)),
    ("nav_build target", F64, (N, 3), lambda e, m, t: e.nav_build(nav(m), field(), None, t)),
    ("nav_query field", U16, (N, GZ, GX), lambda e, m, t: e.nav_query(nav(m), t)),
    ("nav_query pos", F64, (N, 3), lambda e, m, t: e.nav_query(nav(m), field(), pos=t)),
    ("nav_query cost", I32, (N,), lambda e, m, t: e.nav_query(nav(m), field(), cost=t)),
    ("nav_query next", I32, (N,), lambda e, m, t: e.nav_query(nav(m), field(), next=t)),
    ("nav_query waypoint", F64, (N, 2), lambda e, m, t: e.nav_query(nav(m), field(), waypoint=t)),
    ("debug_set_nav_passes", I32, (N,), lambda e, m, t: e.debug_set_nav_passes(t)),
    ("ray_cast t", F64, (N, R), lambda e, m, t: e.ray_cast(ray(m), t)),
    ("ray_cast hit", I32, (N, R), lambda e, m, t: e.ray_cast(ray(m), t_out(), t)),
    ("ray_cast dir_out", F64, (N, R, 2), lambda e, m, t: e.ray_cast(ray(m), t_out(), dir_out=t)),
    ("ray_cast mask", U8, (N,), lambda e, m, t: e.ray_cast(ray(m), t_out(), mask=t)),
    ("ray_cast origin", F64, (N, R, 3), lambda e, m, t: e.ray_cast(ray(m), t_out(), origin=t)),
    ("ray_cast direction", F64, (N, R, 2), lambda e, m, t: e.ray_cast(ray(m), t_out(), direction=t)),
    ("ray_cast offsets", F64, (R,), lambda e, m, t: e.ray_cast(ray(m), t_out(), offsets=t)),
    ("reset_where mask", U8, (N,), lambda e, m, t: e.reset_where(t, make(I64, (N,)))),
    ("reset_where seeds", I64, (N,), lambda e, m, t: e.reset_where(mask(), t)),
    ("set_reset_seeds", I64, (N,), lambda e, m, t: e.set_reset_seeds(t)),
    ("snapshot_save buf", U8, (4096,), lambda e, m, t: e.snapshot_save(t, N)),
    ("snapshot_load buf", U8, (4096,), lambda e, m, t: e.snapshot_load(t, N, N)),
    ("snapshot_save_at buf", U8, (4096,), lambda e, m, t: e.snapshot_save_at(t, N)),
    ("snapshot_load_where buf", U8, (4096,), lambda e, m, t: e.snapshot_load_where(t, N, N, mask(), recs())),
    ("snapshot_load_where mask", U8, (N,), lambda e, m, t: e.snapshot_load_where(buf(), N, N, t, recs())),
    ("snapshot_save_frames buf", U8, (4096,), lambda e, m, t: e.snapshot_save_frames(t, N, obs())),
    ("snapshot_save_frames obs", U8, (N, H, W, 3), lambda e, m, t: e.snapshot_save_frames(buf(), N, t)),
    ("snapshot_save_frames depth", F32, (N, H, W, 1), lambda e, m, t: e.snapshot_save_frames(buf(), N, obs(), t, m.SNAPF_DEPTH)),
    ("snapshot_load_frames buf", U8, (4096,), lambda e, m, t: e.snapshot_load_frames(t, N, N, obs())),
    ("snapshot_load_frames obs", U8, (N, H, W, 3), lambda e, m, t: e.snapshot_load_frames(buf(), N, N, t)),
    ("snapshot_load_frames depth", F32, (N, H, W, 1), lambda e, m, t: e.snapshot_load_frames(buf(), N, N, obs(), t, m.SNAPF_DEPTH)),
    ("snapshot_save_frames_at buf", U8, (4096,), lambda e, m, t: e.snapshot_save_frames_at(t, N, obs())),
    ("snapshot_save_frames_at obs", U8, (N, H, W, 3), lambda e, m, t: e.snapshot_save_frames_at(buf(), N, t)),
    ("snapshot_load_frames_where buf", U8, (4096,), lambda e, m, t: e.snapshot_load_frames_where(t, N, N, mask(), recs(), obs())),
    ("snapshot_load_frames_where mask", U8, (N,), lambda e, m, t: e.snapshot_load_frames_where(buf(), N, N, t, recs(), obs())),
    ("snapshot_load_frames_where obs", U8, (N, H, W, 3), lambda e, m, t: e.snapshot_load_frames_where(buf(), N, N, mask(), recs(), t)),
    ("get_info health", I32, (N,), lambda e, m, t: e.get_info(health=t)),
    ("get_info ent_pos", F64, (N, 3), lambda e, m, t: e.get_info(ent_pos=t)),
    ("get_final_info health", I32, (N,), lambda e, m, t: e.get_final_info(health=t)),
    ("get_final_info goal_pos", F64, (N, 3), lambda e, m, t: e.get_final_info(goal_pos=t)),
    ("get_reset_pending out", U8, (N,), lambda e, m, t: e.get_reset_pending(t)),
    ("get_frame_clean out", U8, (N,), lambda e, m, t: e.get_frame_clean(t)),
    ("get_frame_source out", U8, (N,), lambda e, m, t: e.get_frame_source(t)),
]


def variants(dtype, shape):
    """the right tensor, then the three wrong ones: another dtype, a row short, every second element of a wider one"""
    wide = make(dtype, shape[:-1] + (2 * shape[-1],))
    return [("good", make(dtype, shape)),
            ("wrong dtype", make(OTHER[dtype], shape)),
            ("wrong count", make(dtype, (shape[0] - 1,) + shape[1:])),
            ("non-contiguous", wide[..., ::2])]


def engine_over_the_stub(monkeypatch):
    from miniworld_amd import engine
    from miniworld_amd.scene import base_config
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096, "mw_snapshot_frames_bytes": 4096})
    return engine.Engine(base_config(N, W, H, E, 6, 4, 16)), engine, lib


@pytest.mark.parametrize("label,dtype,shape,call", TABLE, ids=[row[0] for row in TABLE])
def test_a_wrong_tensor_is_refused_before_the_library_is_called(label, dtype, shape, call, monkeypatch):
    e, module, lib = engine_over_the_stub(monkeypatch)
    (_, good), *wrong = variants(dtype, shape)
    for what, t in wrong:
        assert tuple(t.shape) == shape or what == "wrong count"
        assert t.is_contiguous() == (what != "non-contiguous")
        with pytest.raises(module.EngineError):
            call(e, module, t)
        assert [name for name, _ in lib.calls if name not in SIZE_QUERIES] == [], (label, what)
    call(e, module, good)       # (the row itself is right: the same call with the right tensor reaches the library)
    assert [name for name, _ in lib.calls if name not in SIZE_QUERIES] != [], label


def test_converted_arguments_are_still_counted(monkeypatch):
    e, module, lib = engine_over_the_stub(monkeypatch)
    for call in (lambda: e.step(make(I64, (N + 1,)), obs()),
                 lambda: e.step_repeat(make(I64, (N - 1,)), 2, obs()),
                 lambda: e.step_plan(make(I64, (T, N + 1)), obs()),
                 lambda: e.snapshot_save(buf(), N, envs=[0, 1], count=3),
                 lambda: e.snapshot_load_where(buf(), N, N, mask(), [0, 1, 2])):
        with pytest.raises(module.EngineError):
            call()
    assert lib.calls == []
    e.step(make(I64, (2 * N,))[::2], obs())       # a strided int64 action tensor is converted, not refused
    assert [name for name, _ in lib.calls] == ["mw_step"]
