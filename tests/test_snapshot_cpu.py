"""Snapshot records (mw_snapshot_bytes / mw_snapshot_save / mw_snapshot_load), host side, without a GPU: the header declares the three
entry points, the ABI version did not move, the library exports them and refuses a null engine, the record layout
(miniworld_amd/csrc/mw_snapshot.h, compiled for the host from tests/hostcheck/snapshot_layout.cpp) is a partition of the buffer, and
MiniWorldVecEnv.save_state / load_state / fork reach the entry points with the buffers and indices they should."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import stub_engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "snapshot_layout.cpp")
LIB = os.path.join(HERE, "hostcheck", "libmwsnapshot.so")
NAMES = ("mw_snapshot_bytes", "mw_snapshot_save", "mw_snapshot_load")

TASK_GOTO, TASK_PICKUP, TASK_COLLECT = 1, 2, 6
GEN_HALLWAY, GEN_PICKUP, GEN_MAZE, GEN_PROGRAM = 1, 3, 4, 5


def layout_lib():
    """tests/hostcheck/libmwsnapshot.so, (re)built when a source is newer (also used by tests/test_gpu_snapshot.py)."""
    deps = [SRC] + [os.path.join(ROOT, "miniworld_amd", "csrc", h) for h in ("mw_snapshot.h", "mw_world_fields.h", "mw_hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-Wall", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.mwsnap_sections.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mwsnap_bytes.argtypes = [C.c_void_p, C.c_longlong]
    lib.mwsnap_bytes.restype = C.c_longlong
    lib.mwsnap_total_rows.argtypes = [C.c_void_p]
    lib.mwsnap_key.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def snap_config(E, max_polys, max_segs, shared, task, generator, rng_mode, spares):
    """the int32[9] the host check takes: what of an engine's configuration shapes a record"""
    return np.array([max(E, 1), max_polys, max_segs, int(shared), task, generator, rng_mode, int(spares), int(task == TASK_COLLECT)], np.int32)


def sections(lib, cfg, capacity):
    off, size = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    align, ident = np.zeros(64, np.int32), np.zeros(64, np.int32)
    n = lib.mwsnap_sections(cfg.ctypes.data, capacity, off.ctypes.data, size.ctypes.data, align.ctypes.data, ident.ctypes.data, 64)
    assert 0 < n < 64
    return off[:n].astype(np.int64), size[:n].astype(np.int64), align[:n], ident[:n]


def test_header_declares_the_entry_points():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    assert re.search(r"int mw_snapshot_load\(mw_engine \*e, const int32_t \*d_envs, const int32_t \*d_recs, int32_t count,\s*"
                     r"const uint8_t \*d_snap, int32_t n_recs, int32_t capacity, void \*stream\);", header)
    # the comment says what a record leaves out
    for word in ("mw_set_step_params", "frame-stack ring", "per-frame scratch", "shared geometry set"):
        assert word in header, word
    layout = open(os.path.join(ROOT, "miniworld_amd", "csrc", "mw_snapshot.h")).read()
    assert "NOT part of a record" in layout and "mw_set_step_params" in layout


def test_library_exports_the_entry_points_and_refuses_a_null_engine():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    buf = (C.c_uint8 * 256)()
    assert lib.mw_snapshot_bytes(None, 4) == -1                      # no engine: MW_E_INVALID
    assert lib.mw_snapshot_save(None, None, 1, C.cast(buf, C.c_void_p), 4, None) == -1
    assert lib.mw_snapshot_load(None, None, None, 1, C.cast(buf, C.c_void_p), 1, 4, None) == -1
    assert not any(buf)
    assert lib.mw_abi_version() == 4


CONFIGS = {
    "hallway, spares": snap_config(1, 6, 4, True, TASK_GOTO, GEN_HALLWAY, 1, True),
    "hallway, no spares": snap_config(1, 6, 4, True, TASK_GOTO, GEN_HALLWAY, 0, False),
    "maze, spares": snap_config(1, 510, 256, False, TASK_GOTO, GEN_MAZE, 1, True),
    "mazeS2": snap_config(1, 30, 16, False, TASK_GOTO, GEN_MAZE, 1, True),
    "pickup, own geometry": snap_config(5, 6, 4, False, TASK_PICKUP, GEN_PICKUP, 1, False),
    "collecthealth": snap_config(19, 6, 4, True, TASK_COLLECT, GEN_PROGRAM, 1, False),
    "64 slots, odd capacities": snap_config(64, 7, 3, False, TASK_GOTO, GEN_PROGRAM, 1, True),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("capacity", [0, 1, 3, 70, 1023, 4096])
def test_the_layout_is_a_partition_of_the_buffer(name, capacity):
    """Sections in address order: the first starts behind the header, each starts where the one before ends (disjoint, no holes),
    each is aligned for the copies made of it — 16 bytes for the blobs, the element size for the components —, and the end of the
    last one, in whole 16-byte units, is the size mw_snapshot_bytes reports (it returns this very function's value)."""
    lib, cfg = layout_lib(), CONFIGS[name]
    off, size, align, ident = sections(lib, cfg, capacity)
    order = np.argsort(off, kind="stable")
    assert lib.mwsnap_header_bytes() == 64
    end = 64
    for k in order:
        assert off[k] == end, (name, capacity, int(ident[k]), "starts", int(off[k]), "expected", end)
        assert off[k] % align[k] == 0, (name, capacity, int(ident[k]), "misaligned")
        end = off[k] + size[k]
    total = lib.mwsnap_bytes(cfg.ctypes.data, capacity)
    assert total == (end + 15) // 16 * 16 and total % 16 == 0
    shared, spares, E, health = bool(cfg[3]), bool(cfg[7]), int(cfg[0]), bool(cfg[8])
    # blobs exist with per-env geometry alone, twice with spares; and the components are the ones the issue lists
    assert (ident < 0).sum() == (0 if shared else 4 if spares else 2)
    live_rows = 4 + 4 + 12 + 4 + 3 + 2 * health + 3 + 16 * E + 5 + 1 + 1 + (0 if shared else 2)
    spare_rows = (4 + 4 + 12 + 4 + 16 * E + (0 if shared else 2) + 1) if spares else 0
    assert lib.mwsnap_total_rows(cfg.ctypes.data) == live_rows + spare_rows


def test_the_key_tells_configurations_apart():
    lib = layout_lib()

    def key(cfg, capacity):
        out = np.zeros(12, np.uint32)
        lib.mwsnap_key(cfg.ctypes.data, capacity, out.ctypes.data)
        return tuple(out)
    base = snap_config(5, 6, 4, False, TASK_PICKUP, GEN_PICKUP, 1, True)
    keys = {key(base, 9)}
    for field in range(8):          # E, max_polys, max_segs, shared_geometry, task, generator, rng_mode, spares
        other = base.copy()
        other[field] = 1 - other[field] if field in (3, 6, 7) else other[field] + 1
        keys.add(key(other, 9))
    keys.add(key(base, 10))         # the capacity the buffer was laid out for
    assert len(keys) == 10
    assert key(base, 9)[1] == 1     # the format number


def _val(x):
    return None if x is None else x.value


def test_vec_env_reaches_the_entry_points(monkeypatch):
    import torch
    from miniworld_amd.vec_env import EnvSnapshot, MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-Hallway-v0", 5, frame_stack=2)
    snap = vec.save_state()
    assert isinstance(snap, EnvSnapshot) and (snap.count, snap.capacity) == (5, 5) and len(snap) == 5
    assert snap.data.dtype == torch.uint8 and snap.data.numel() == 4096
    name, args = lib.calls[-1]
    assert name == "mw_snapshot_save" and args[1] is None and args[2] == 5 and args[3].value == snap.data.data_ptr() and args[4] == 5
    part = vec.save_state([3, 1])
    name, args = lib.calls[-1]
    assert (part.count, part.capacity) == (2, 2) and args[1] is not None and args[2] == 2 and args[4] == 2
    one = vec.save_state([3], capacity=5)       # one record in a buffer laid out for five: loadable into five envs at once
    name, args = lib.calls[-1]
    assert (one.count, one.capacity) == (1, 5) and args[2] == 1 and args[4] == 5
    with pytest.raises(ValueError):
        vec.save_state([3, 1], capacity=1)
    # load: the call, then the reset path's frame and stack refresh; returns the observation tensor
    n0 = len(lib.calls)
    out = vec.load_state(snap, envs=[2, 4], records=torch.tensor([0, 0]))
    assert out is vec.obs
    assert [c[0] for c in lib.calls[n0:]] == ["mw_snapshot_bytes", "mw_snapshot_load", "mw_render", "mw_stack_refresh"]
    args = lib.calls[n0 + 1][1]
    assert args[1] is not None and args[2] is not None and args[3] == 2 and args[4].value == snap.data.data_ptr() and args[5:7] == (5, 5)
    n0 = len(lib.calls)
    vec.load_state(snap)
    args = lib.calls[n0 + 1][1]
    assert args[1] is None and args[2] is None and args[3] == 5
    # fork: a whole-batch save into the env's own scratch records, a load through src
    n0 = len(lib.calls)
    out = vec.fork(torch.tensor([1, 1, 0, 3, 4]))
    assert out is vec.obs
    names = [c[0] for c in lib.calls[n0:] if c[0] != "mw_snapshot_bytes"]
    assert names == ["mw_snapshot_save", "mw_snapshot_load", "mw_render", "mw_stack_refresh"]
    save, load = [c[1] for c in lib.calls[n0:] if c[0] in ("mw_snapshot_save", "mw_snapshot_load")]
    assert save[1] is None and save[2] == 5 and save[4] == 5 and save[3].value == load[4].value == vec._fork_buf.data_ptr()
    assert load[1] is None and load[2] is not None and load[3] == 5 and load[5:7] == (5, 5)
    with pytest.raises(Exception):
        vec.fork(torch.tensor([0, 1]))      # one source per env
    # a snapshot travels: .cpu() / .to() keep the counts, the state dict round-trips
    moved = EnvSnapshot.from_state_dict(snap.cpu().state_dict())
    assert (moved.count, moved.capacity) == (5, 5) and torch.equal(moved.data, snap.data)
    # the Gymnasium adapter gained nothing
    from miniworld_amd.vector import MiniWorldVectorEnv
    assert not any(hasattr(MiniWorldVectorEnv, n) for n in ("save_state", "load_state", "fork"))
