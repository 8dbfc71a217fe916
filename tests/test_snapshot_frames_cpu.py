"""Frame records (mw_snapshot_frames_bytes / mw_snapshot_save_frames / mw_snapshot_load_frames), host side, without a GPU: the header
declares the three entry points, the ABI version did not move, the library exports them and refuses a null engine, the record layout
(miniworld_amd/csrc/mw_snapframes.h, compiled for the host from tests/hostcheck/snapframes_layout.cpp) is a partition of the buffer,
MiniWorldVecEnv.save_state / load_state / fork reach the entry points in the documented order, and an EnvSnapshot carries its frames."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import stub_engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "snapframes_layout.cpp")
LIB = os.path.join(HERE, "hostcheck", "libmwsnapframes.so")
NAMES = ("mw_snapshot_frames_bytes", "mw_snapshot_save_frames", "mw_snapshot_load_frames")
SNAPF_DEPTH, SNAPF_STACK = 1, 2
HWC, CWH, GREY = 0, 1, 2
SF_OBS, SF_DEPTH, SF_STACK, SF_STACK_FLAG = 0, 1, 2, 3


def layout_lib():
    """tests/hostcheck/libmwsnapframes.so, (re)built when a source is newer (also used by tests/test_gpu_snapshot_frames.py)."""
    deps = [SRC] + [os.path.join(ROOT, "miniworld_amd", "csrc", h) for h in ("mw_snapframes.h", "mw_hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-Wall", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.mwsnapf_sections.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mwsnapf_bytes.argtypes = [C.c_void_p, C.c_longlong]
    lib.mwsnapf_bytes.restype = C.c_longlong
    lib.mwsnapf_key.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def frames_config(W, H, layout, flags, K):
    """the int64[6] the host check takes: W, H, obs layout, flags, stack depth, bytes of a frame"""
    return np.array([W, H, layout, flags, K, W * H * (8 if layout == GREY else 3)], np.int64)


def sections(lib, cfg, capacity):
    off, size, rec = np.zeros(8, np.uint64), np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    ident = np.zeros(8, np.int32)
    n = lib.mwsnapf_sections(cfg.ctypes.data, capacity, off.ctypes.data, size.ctypes.data, rec.ctypes.data, ident.ctypes.data, 8)
    return off[:n].astype(np.int64), size[:n].astype(np.int64), rec[:n].astype(np.int64), ident[:n]


def test_header_declares_the_entry_points():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"enum \{ MW_SNAPF_DEPTH = 1, MW_SNAPF_STACK = 2 \};", header)
    assert re.search(r"int mw_snapshot_save_frames\(mw_engine \*e, const int32_t \*d_envs, int32_t count, const uint8_t \*d_obs, const float \*d_depth,\s*"
                     r"uint8_t \*d_frames, int32_t capacity, int32_t flags, void \*stream\);", header)
    assert re.search(r"int mw_snapshot_load_frames\(mw_engine \*e, const int32_t \*d_envs, const int32_t \*d_recs, int32_t count, const uint8_t \*d_frames,\s*"
                     r"int32_t n_recs, int32_t capacity, int32_t flags, uint8_t \*d_obs, float \*d_depth, void \*stream\);", header)
    assert (engine.SNAPF_DEPTH, engine.SNAPF_STACK) == (SNAPF_DEPTH, SNAPF_STACK)
    # a STATE record still holds no frames, and the header still says so; the frame record's comment says what its obs row is
    assert "rendered frames and the frame-stack ring" in header
    assert "whatever the row holds" in header


def test_library_exports_the_entry_points_and_refuses_a_null_engine():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    buf, obs = (C.c_uint8 * 256)(), (C.c_uint8 * 64)()
    p, o = C.cast(buf, C.c_void_p), C.cast(obs, C.c_void_p)
    assert lib.mw_snapshot_frames_bytes(None, 4, 0) == -1            # no engine: MW_E_INVALID
    assert lib.mw_snapshot_save_frames(None, None, 1, o, None, p, 4, 0, None) == -1
    assert lib.mw_snapshot_load_frames(None, None, None, 1, p, 1, 4, 0, o, None, None) == -1
    assert not any(buf) and not any(obs)
    assert lib.mw_abi_version() == 4


FRAMES = {"80x60x3": (80, 60, HWC), "81x61x3": (81, 61, HWC), "80x60 grey f64": (80, 60, GREY), "1x1x3": (1, 1, HWC)}


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("flags", [0, SNAPF_DEPTH, SNAPF_STACK, SNAPF_DEPTH | SNAPF_STACK])
@pytest.mark.parametrize("capacity", [0, 1, 3, 70, 4096])
def test_the_layout_is_a_partition_of_the_buffer(frame, flags, capacity):
    """Sections in address order: the first starts behind the 64-byte header, each starts where the one before ends (disjoint, no
    holes), each starts 16-byte aligned and holds its `capacity` records back to back (a frame is contiguous), and the end of the last
    one is the size mw_snapshot_frames_bytes reports (it returns this very function's value)."""
    lib = layout_lib()
    W, H, layout = FRAMES[frame]
    fb = W * H * (8 if layout == GREY else 3)
    assert lib.mwsnapf_header_bytes() == 64
    for K in (2, 3, 16) if flags & SNAPF_STACK else (0,):
        cfg = frames_config(W, H, layout, flags, K)
        off, size, rec, ident = sections(lib, cfg, capacity)
        want = {SF_OBS: fb}
        if flags & SNAPF_DEPTH:
            want[SF_DEPTH] = W * H * 4
        if flags & SNAPF_STACK:
            want[SF_STACK], want[SF_STACK_FLAG] = K * fb, 1
        assert dict(zip(ident.tolist(), rec.tolist())) == want, (frame, flags, K)
        end = 64
        for k in np.argsort(off, kind="stable"):
            assert off[k] == end, (frame, flags, K, capacity, int(ident[k]), "starts", int(off[k]), "expected", end)
            assert off[k] % 16 == 0 and size[k] % 16 == 0, (frame, flags, K, capacity, int(ident[k]), "misaligned")
            assert rec[k] * capacity <= size[k] < rec[k] * capacity + 16, (frame, flags, K, capacity, int(ident[k]), "not its records, padded to 16")
            end = off[k] + size[k]
        assert lib.mwsnapf_bytes(cfg.ctypes.data, capacity) == end


def test_the_key_tells_configurations_apart():
    lib = layout_lib()

    def key(cfg, capacity):
        out = np.zeros(12, np.uint32)
        lib.mwsnapf_key(cfg.ctypes.data, capacity, out.ctypes.data)
        return tuple(out)
    base = frames_config(80, 60, HWC, SNAPF_DEPTH | SNAPF_STACK, 3)
    keys = {key(base, 9)}
    for field, other_value in ((0, 81), (1, 61), (2, CWH), (3, SNAPF_STACK), (4, 4), (5, 14401)):   # W, H, layout, flags, K, frame bytes
        other = base.copy()
        other[field] = other_value
        keys.add(key(other, 9))
    keys.add(key(base, 10))         # the capacity the buffer was laid out for
    assert len(keys) == 8
    assert key(base, 9)[1] == 1     # the format number
    # the stack depth counts with MW_SNAPF_STACK alone
    assert key(frames_config(80, 60, HWC, 0, 3), 9) == key(frames_config(80, 60, HWC, 0, 5), 9)


def _val(x):
    return None if x is None else x.value


def _names(calls):
    return [c[0] for c in calls if c[0] not in ("mw_snapshot_bytes", "mw_snapshot_frames_bytes")]


@pytest.mark.parametrize("want_depth,frame_stack,flags", [(False, None, 0), (True, None, SNAPF_DEPTH), (False, 2, SNAPF_STACK),
                                                          (True, 3, SNAPF_DEPTH | SNAPF_STACK)])
def test_vec_env_reaches_the_entry_points(monkeypatch, want_depth, frame_stack, flags):
    import torch
    from miniworld_amd.vec_env import EnvSnapshot, MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5, want_depth=want_depth, frame_stack=frame_stack)
    depth_ptr = vec.depth.data_ptr() if want_depth else None
    # save: the state records, then the frame records, from vec.obs / vec.depth under the flags of this env
    n0 = len(lib.calls)
    snap = vec.save_state(frames=True)
    assert isinstance(snap, EnvSnapshot) and (snap.count, snap.capacity) == (5, 5)
    assert snap.frames is not None and snap.frames.dtype == torch.uint8 and (snap.frame_flags, snap.frame_stack) == (flags, frame_stack or 0)
    assert _names(lib.calls[n0:]) == ["mw_snapshot_save", "mw_snapshot_save_frames"]
    args = lib.calls[-1][1]
    assert args[1] is None and args[2] == 5 and args[3].value == vec.obs.data_ptr() and _val(args[4]) == depth_ptr
    assert _val(args[5]) == (snap.frames.data_ptr() or None) and args[6:8] == (5, flags)
    part = vec.save_state([3, 1], capacity=4, frames=True)
    args = lib.calls[-1][1]
    assert (part.count, part.capacity) == (2, 4) and args[1] is not None and args[2] == 2 and args[6:8] == (4, flags)
    # load: the two copies and nothing drawn, nothing rebuilt; the same index arrays for both
    n0 = len(lib.calls)
    out = vec.load_state(snap, envs=[2, 4], records=torch.tensor([0, 0]))
    assert out is vec.obs
    assert _names(lib.calls[n0:]) == ["mw_snapshot_load", "mw_snapshot_load_frames"]
    load, loadf = [c[1] for c in lib.calls[n0:] if c[0] in ("mw_snapshot_load", "mw_snapshot_load_frames")]
    assert load[1].value == loadf[1].value and load[2].value == loadf[2].value and load[3] == loadf[3] == 2
    assert _val(loadf[4]) == (snap.frames.data_ptr() or None) and loadf[5:8] == (5, 5, flags)
    assert loadf[8].value == vec.obs.data_ptr() and _val(loadf[9]) == depth_ptr
    n0 = len(lib.calls)
    vec.load_state(snap, frames=True)
    loadf = lib.calls[-1][1]
    assert _names(lib.calls[n0:]) == ["mw_snapshot_load", "mw_snapshot_load_frames"] and loadf[1] is None and loadf[2] is None and loadf[3] == 5
    # frames=False on the same snapshot, and a snapshot without frames: the redraw path exactly
    redraw = ["mw_snapshot_load", "mw_render"] + (["mw_stack_refresh"] if frame_stack else [])
    for s, kw in ((snap, {"frames": False}), (vec.save_state(), {})):
        n0 = len(lib.calls)
        assert vec.load_state(s, envs=[2, 4], records=[0, 0], **kw) is vec.obs
        assert [c[0] for c in lib.calls[n0:]] == ["mw_snapshot_bytes"] + redraw
    # fork: save, save_frames, load, load_frames through src into scratch of the env's own
    n0 = len(lib.calls)
    out = vec.fork(torch.tensor([1, 1, 0, 3, 4]), frames=True)
    assert out is vec.obs
    assert _names(lib.calls[n0:]) == ["mw_snapshot_save", "mw_snapshot_save_frames", "mw_snapshot_load", "mw_snapshot_load_frames"]
    save, savef, load, loadf = [c[1] for c in lib.calls[n0:] if c[0] not in ("mw_snapshot_bytes", "mw_snapshot_frames_bytes")]
    assert save[1] is None and save[2] == 5 and save[3].value == load[4].value == vec._fork_buf.data_ptr()
    assert savef[1] is None and savef[2] == 5 and savef[3].value == vec.obs.data_ptr() and savef[6:8] == (5, flags)
    assert _val(savef[5]) == _val(loadf[4]) == (vec._fork_frames.data_ptr() or None)
    assert load[1] is None and loadf[1] is None and load[2].value == loadf[2].value and load[3] == loadf[3] == 5
    assert loadf[5:8] == (5, 5, flags) and loadf[8].value == vec.obs.data_ptr() and _val(loadf[9]) == depth_ptr
    n0 = len(lib.calls)
    vec.fork(torch.tensor([1, 1, 0, 3, 4]))
    assert _names(lib.calls[n0:]) == ["mw_snapshot_save"] + redraw


def test_load_state_refuses_on_the_host(monkeypatch):
    from miniworld_amd.vec_env import MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    two = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5, frame_stack=2)
    three = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5, frame_stack=3)
    plain = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5)
    deep = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5, want_depth=True)
    old, with_two = two.save_state(), two.save_state(frames=True)
    n0 = len(lib.calls)
    with pytest.raises(ValueError):
        two.load_state(old, frames=True)            # no frames in the snapshot
    with pytest.raises(ValueError):
        three.load_state(with_two)                  # K = 2 into K = 3
    with pytest.raises(ValueError):
        plain.load_state(with_two)                  # stacks into an env without one
    with pytest.raises(ValueError):
        deep.load_state(plain.save_state(frames=True), frames=True)     # no depth rows for an env with depth
    launched = [c[0] for c in lib.calls[n0:] if "load" in c[0] or c[0] in ("mw_render", "mw_stack_refresh")]
    assert launched == [], launched
    three.load_state(with_two, frames=False)        # the states alone are compatible


def test_a_snapshot_carries_its_frames():
    import torch
    from miniworld_amd.vec_env import EnvSnapshot
    data, frames = torch.arange(64, dtype=torch.uint8), torch.arange(96, dtype=torch.uint8) + 100
    snap = EnvSnapshot(data, 3, 4, frames, SNAPF_DEPTH | SNAPF_STACK, 3)
    twin = snap.clone()
    assert twin.frames is not snap.frames and twin.frames.data_ptr() != snap.frames.data_ptr()
    for other in (snap.cpu(), twin, snap.to("cpu"), EnvSnapshot.from_state_dict(snap.state_dict())):
        assert (other.count, other.capacity, other.frame_flags, other.frame_stack) == (3, 4, 3, 3)
        assert torch.equal(other.data, data) and torch.equal(other.frames, frames)
    assert set(snap.state_dict()) == {"data", "count", "capacity", "frames", "frame_flags", "frame_stack"}
    # ... and one without frames is what it was: the state dict of before loads, and has the keys of before
    old = EnvSnapshot.from_state_dict({"data": data, "count": 3, "capacity": 4})
    assert old.frames is None and (old.frame_flags, old.frame_stack) == (0, 0) and len(old) == 3
    assert set(old.state_dict()) == {"data", "count", "capacity"}
    assert old.clone().frames is None and old.cpu().frames is None
