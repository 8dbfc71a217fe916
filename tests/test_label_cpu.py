"""Label frames (mw_label_frame; MiniWorldVecEnv.label_frame / label_update) without a GPU.

The phases the kernel runs (miniworld_amd/csrc/mw_label.h) — the staged polygons and slots, the triangle-per-worker mesh phase with its
pruning rectangle, the bands — run on the host with (lane, stride) = (0, 1) in a program of its own (tests/hostcheck/label_frame.cpp), built
with the address and undefined-behaviour sanitizers, on worlds the host classes generate; all five outputs over short walks are compared,
exactly, with the brute-force restatement of tests/label_reference.py.  The definition itself is checked against the renderer: at the
interior pixels of the oracle's own frames of the same states the label's eye depth lies within the frame's 16-bit depth value +- 2
steps.  Beside that: the check's sharpness, bounds against exact, the statistics, the ABI names, the launch arithmetic, the refusals of
the binding over a stub engine and the adapter's key."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import label_reference as ref
from helpers import golden_meshes, stub_engine
from query_checks import (CSRC, ROOT, build, check_does_not_wait, check_kernel, check_refuses_null_engine, check_units_built, launch_of, run,
                          scene as _scene, scene_walk)
from test_depth_cpu import CAMERAS

FAMILIES = ["Hallway", "OneRoom", "MazeS3", "FourRooms", "Sign", "PickupObjects", "Sidewalk", "CollectHealth"]
BOUNDS, UNPRUNED = 1, 2
# the caps of the renderer check (the issue's): misses among a frame's interior pixels, and interior pixels of a frame
MISS_CAP, INTERIOR_FLOOR = 0.005, 0.70


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build("label_frame", tmp_path_factory.mktemp("label_frame"))


_frames, _labels = {}, {}


def _poses(cls_name, steps, seed=0):
    """poses (x, y, z, dir) from the world's own first one: turns of 40 degrees and forward moves, kept inside the extent"""
    y = float(_scene(cls_name, seed)["agent_pos"][1])
    return [(x, y, z, d) for x, z, d in scene_walk(cls_name, steps, seed, 3500 + seed, 40)]


def _posed(sc, pose, cam):
    sc = dict(sc)
    sc["agent_pos"], sc["agent_dir"] = np.array(pose[:3], np.float64), np.float64(pose[3])
    sc["cam_height"], sc["cam_fwd_disp"], sc["cam_pitch"], sc["cam_fov_y"] = cam
    return sc


def _label(sc, key, pose, cam, msaa, W, H, mode="exact", **kw):
    """the restatement's frame, computed once per key and never changed"""
    key = (key, pose, cam, msaa, W, H, mode, tuple(sorted(kw.items())))
    if key not in _labels:
        out = ref.label_frame(sc, W, H, msaa, meshes=golden_meshes(sc), mode=mode, pose=pose, cam=cam, **kw)
        for v in out.values():
            v.setflags(write=False)
        _labels[key] = out
    return _labels[key]


def _render(sc, key, pose, cam, msaa, W, H):
    key = (key, pose, cam, msaa, W, H)
    if key not in _frames:
        import pyoracle
        out = pyoracle.render(_posed(sc, pose, cam), W, H, msaa, meshes=golden_meshes(sc))
        _frames[key] = out["z16"].copy()
        _frames[key].setflags(write=False)
    return _frames[key]


def _hex(a):
    return " ".join(f"{v:x}" for v in np.ascontiguousarray(a, np.float32).ravel().view(np.uint32).tolist())


def _run(program, tmp_path, sc, W, H, msaa, steps, flags=0, near=ref.NEAR, far=ref.FAR, band_rows=0, chunk=0, garbage=0xAB):
    """steps: (pose, cam, mask) -> per step dict(cls, code, depth, ent_pixels, ent_box) of the host build"""
    meshes = golden_meshes(sc)
    names = [str(n) for n in sc.get("mesh_names", [])]
    P, E = len(sc["polys_nv"]), len(sc["ents_kind"])
    lines = [f"{W} {H} {msaa} {float(near)!r} {float(far)!r} {flags} {band_rows} {chunk}", str(P)]
    for i in range(P):
        lines.append(f"{int(sc['polys_nv'][i])} {_hex(sc['polys_v'][i])} {_hex(sc['polys_xf'][i])}")
    lines.append(str(E))
    for s in range(E):
        geom = list(sc["ents_size"][s]) + list(sc["ents_color"][s]) + [sc["ents_scale"][s], sc["ents_radius"][s], sc["ents_height"][s]]
        vals = list(sc["ents_pos"][s]) + [sc["ents_dir"][s]] + geom
        lines.append(f"{int(sc['ents_kind'][s])} {int(sc['ents_mesh'][s])} " + " ".join(repr(float(v)) for v in vals))
    lines.append(str(len(names)))
    for n in names:
        v = np.asarray(meshes[n]["verts"], np.float32)
        lines.append(f"{v.shape[0]} {_hex(v)}")
    lines += [str(garbage), str(len(steps))]
    for pose, cam, mask in steps:
        lines.append(" ".join(repr(float(v)) for v in tuple(pose) + tuple(cam)) + f" {int(mask)}")
    rows = run(program, tmp_path / "scene.txt", lines, timeout=600, blank=True)
    assert len(rows) == 5 * len(steps)
    out = []
    for k in range(len(steps)):
        c, co, d, px, bx = rows[5 * k:5 * k + 5]
        out.append(dict(cls=np.array(c.split(), np.uint8).reshape(H, W), code=np.array(co.split(), np.int64).astype(np.int32).reshape(H, W),
                        depth=np.array([int(v, 16) for v in d.split()], np.uint32).view(np.float32).reshape(H, W),
                        ent_pixels=np.array(px.split(), np.int64).astype(np.int32), ent_box=np.array(bx.split(), np.int64).astype(np.int32).reshape(E, 4)))
    return out


def _same(got, want, what):
    for k in ("cls", "code", "ent_pixels", "ent_box"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:8].tolist())
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32)), (what, "depth", np.argwhere(got["depth"] != want["depth"])[:8].tolist())


# (msaa, W, H, band_rows): the frame formats of the walks; band_rows 0 = the launch policy's (one band), else several bands with a ragged last one
FORMATS = [(8, 80, 60, 0), (4, 81, 61, 0), (1, 21, 13, 0), (8, 81, 61, 17), (4, 80, 60, 0), (1, 80, 60, 7)]


@pytest.mark.parametrize("cls_name", FAMILIES)
def test_program_equals_the_restatement(program, tmp_path, cls_name):
    sc = _scene(cls_name)
    poses = _poses(cls_name, 6)
    has_mesh = any(int(k) == ref.ENT_MESH for k in sc["ents_kind"])
    seen = set()
    for k, pose in enumerate(poses):
        msaa, W, H, band = FORMATS[k % len(FORMATS)]
        cam = CAMERAS[k % len(CAMERAS)]
        # polygons in chunks of 5 on every other pose (a scene of few polygons takes the chunk loop too)
        for mode, flags in (("exact", 0), ("bounds", BOUNDS)) if has_mesh else (("exact", 0),):
            got = _run(program, tmp_path, sc, W, H, msaa, [(pose, cam, 1)], flags=flags, band_rows=band, chunk=5 if k % 2 else 0)[0]
            want = _label(sc, cls_name, pose, cam, msaa, W, H, mode)
            _same(got, want, (cls_name, k, mode))
            seen |= set(np.unique(want["cls"]).tolist())
    assert ref.WALL in seen and ref.FLOOR in seen, seen
    if has_mesh:
        assert ref.MESH in seen, seen


def test_masked_step_keeps_every_byte_and_other_ranges(program, tmp_path):
    sc = _scene("PickupObjects")
    pose, cam = _poses("PickupObjects", 1)[0], CAMERAS[0]
    got = _run(program, tmp_path, sc, 21, 13, 8, [(pose, cam, 0), (pose, cam, 1)], garbage=0x5A)
    assert (got[0]["cls"] == 0x5A).all() and (got[0]["code"] == 0x5A5A5A5A).all() and (got[0]["ent_box"] == 0x5A5A5A5A).all()
    _same(got[1], _label(sc, "PickupObjects", pose, cam, 8, 21, 13), "after the mask")
    # a near and far of the caller's: what lies outside shows nothing, far is the depth of nothing
    near, far = 1.5, 4.0
    got = _run(program, tmp_path, sc, 80, 60, 8, [(pose, cam, 1)], near=near, far=far)[0]
    want = _label(sc, "PickupObjects", pose, cam, 8, 80, 60, near=near, far=far)
    _same(got, want, "near / far")
    assert (want["code"] < 0).any() and (want["code"] >= 0).any() and (want["depth"][want["code"] < 0] == np.float32(far)).all()
    assert (want["depth"][want["code"] >= 0] >= np.float32(near)).all()
    # a NaN pose: nothing anywhere
    nan = float("nan")
    got = _run(program, tmp_path, sc, 21, 13, 8, [((nan, 0.0, 1.0, 0.3), cam, 1)])[0]
    assert (got["cls"] == 0).all() and (got["code"] == -1).all() and (got["depth"] == np.float32(ref.FAR)).all() and not got["ent_pixels"].any()


def _carried_scene():
    """RoomObjects with the first mesh slot carried: where Agent.step puts it, in front of the camera (miniworld.py:700-712)"""
    sc = dict(_scene("RoomObjects"))
    slot = [int(k) for k in sc["ents_kind"]].index(ref.ENT_MESH)
    pos, d = np.asarray(sc["agent_pos"], np.float64), float(sc["agent_dir"])
    ents_pos = np.array(sc["ents_pos"], np.float64)
    reach = 0.4 + float(sc["ents_radius"][slot]) + 0.17
    ents_pos[slot] = (pos[0] + reach * math.cos(d), 1.5 - 0.4, pos[2] - reach * math.sin(d))
    sc["ents_pos"], sc["agent_carrying"] = ents_pos, np.int32(slot)
    return sc, slot


def _inside_scene():
    """PickupObjects with the agent standing inside the first mesh slot's cylinder: triangles on both sides of the eye plane"""
    sc = dict(_scene("PickupObjects"))
    slot = [int(k) for k in sc["ents_kind"]].index(ref.ENT_MESH)
    pos = np.array(sc["agent_pos"], np.float64)
    pos[0], pos[2] = float(sc["ents_pos"][slot][0]) + 0.02, float(sc["ents_pos"][slot][2]) - 0.01
    sc["agent_pos"] = pos
    return sc, slot


@pytest.mark.parametrize("which", ["carried", "inside"])
def test_near_plane_fallback_equals_brute_force(program, tmp_path, which):
    sc, slot = _carried_scene() if which == "carried" else _inside_scene()
    pose = tuple(float(v) for v in sc["agent_pos"]) + (float(sc["agent_dir"]),)
    cam = CAMERAS[0] if which == "carried" else (0.05, 0.0, 20.0, 60.0)         # (inside: an eye low enough to lie within the mesh's height, looking up)
    W, H = 40, 30
    want = ref.label_frame(sc, W, H, 8, meshes=golden_meshes(sc), pose=pose, cam=cam, select="all")
    pruned = _run(program, tmp_path, sc, W, H, 8, [(pose, cam, 1)])[0]
    brute = _run(program, tmp_path, sc, W, H, 8, [(pose, cam, 1)], flags=UNPRUNED)[0]
    _same(pruned, want, which)
    _same(brute, want, which + ", unpruned")
    _same({k: v for k, v in ref.label_frame(sc, W, H, 8, meshes=golden_meshes(sc), pose=pose, cam=cam).items() if k != "t"}, want, "the restatement's sphere")
    print(f"{which}: slot {slot} shows in {int(want['ent_pixels'][slot])} of {W * H} pixels")
    if which == "carried":
        assert want["ent_pixels"][slot] > 20         # it is drawn, so it is labelled


# ---------------------------------------------------------------------------------------------------------------- the renderer

# (family, pose of its walk, camera, msaa, W, H): frames for which the restatement alone stays inside both caps
# (a pose given in full: the Sign's frame, which the walk never faces; no 21 x 13 frame: of its 273 pixels some 55 % are interior)
RENDERED = [("Hallway", 0, 0, 8, 80, 60), ("OneRoom", 1, 1, 4, 80, 60), ("MazeS3", 0, 2, 8, 81, 61), ("FourRooms", 2, 3, 1, 80, 60), ("Sign", 0, 0, 8, 84, 84),
            ("Sign", (8.5, 0.0, 9.0, -0.7), 1, 8, 80, 60), ("PickupObjects", 0, 4, 8, 80, 60), ("Sidewalk", 2, 0, 8, 80, 60), ("Sidewalk", 5, 2, 1, 80, 60),
            ("CollectHealth", 1, 1, 8, 80, 60), ("PickupObjects", 3, 0, 4, 81, 61)]


def _renderer_check(cls_name, k, cam, msaa, W, H, label_of=None):
    sc = _scene(cls_name)
    pose = k if isinstance(k, tuple) else _poses(cls_name, 6)[k]
    z16 = _render(sc, cls_name, pose, cam, msaa, W, H)
    label = label_of(sc, pose, cam) if label_of else _label(sc, cls_name, pose, cam, msaa, W, H)
    return ref.against_frame(label, z16) + (label,)


def test_labels_are_the_renderers():
    seen = set()
    for cls_name, k, c, msaa, W, H in RENDERED:
        bad, inner, label = _renderer_check(cls_name, k, CAMERAS[c], msaa, W, H)
        print(f"{cls_name} pose {k} cam {c} msaa {msaa} {W}x{H}: {bad} of {inner} interior pixels miss, {inner} of {W * H} interior")
        assert inner >= INTERIOR_FLOOR * W * H, (cls_name, k, inner)
        assert bad <= MISS_CAP * inner, (cls_name, k, bad, inner)
        seen |= set(np.unique(label["cls"]).tolist())
    assert seen == set(range(7)), seen


def test_the_check_is_sharp():
    """each wrong definition pushes one chosen frame over the cap"""
    cam = CAMERAS[2]

    def over(cls_name, k, msaa, label_of, cam=cam):
        good, inner, _ = _renderer_check(cls_name, k, cam, msaa, 80, 60)
        bad, inner_bad, _ = _renderer_check(cls_name, k, cam, msaa, 80, 60, label_of)
        print(f"{cls_name}: {good} of {inner} miss as defined, {bad} of {inner_bad} with the wrong definition")
        assert good <= MISS_CAP * inner and bad > MISS_CAP * inner_bad, (cls_name, good, inner, bad, inner_bad)

    # the pixel's centre in place of sample 0 (1 sample: the centre), and a flipped pitch
    over("OneRoom", 0, 8, lambda sc, pose, cam: ref.label_frame(sc, 80, 60, 1, meshes=golden_meshes(sc), pose=pose, cam=cam))
    over("OneRoom", 0, 8, lambda sc, pose, cam: ref.label_frame(sc, 80, 60, 8, meshes=golden_meshes(sc), pose=pose, cam=(cam[0], cam[1], -cam[2], cam[3])))

    # a Box turned by -dir
    def turned(sc, pose, cam):
        sc = dict(sc)
        sc["ents_dir"] = -np.asarray(sc["ents_dir"], np.float64)
        return ref.label_frame(sc, 80, 60, 8, meshes=golden_meshes(sc), pose=pose, cam=cam)

    # a mesh scaled after the translation instead of before it
    def scaled(sc, pose, cam):
        sc = dict(sc)
        sc["ents_pos"] = np.asarray(sc["ents_pos"], np.float64) * np.asarray(sc["ents_scale"], np.float64)[:, None]
        return ref.label_frame(sc, 80, 60, 8, meshes=golden_meshes(sc), pose=pose, cam=cam)

    sc = _scene("Hallway")
    box = np.asarray(sc["ents_pos"][0], np.float64)
    close = (float(box[0]) - 2.5, 0.0, float(box[2]) + 0.1, 0.0)         # the Hallway's box from 2.5 m: some 300 pixels of it
    z16 = _render(sc, "Hallway", close, CAMERAS[0], 8, 80, 60)
    good = ref.against_frame(ref.label_frame(sc, 80, 60, 8, pose=close, cam=CAMERAS[0]), z16)
    bad = ref.against_frame(turned(sc, close, CAMERAS[0]), z16)
    print(f"Hallway box: {good} as defined, {bad} turned by -dir")
    assert good[0] <= MISS_CAP * good[1] and bad[0] > MISS_CAP * bad[1]
    sc = _scene("PickupObjects")
    slot = [int(k) for k in sc["ents_kind"]].index(ref.ENT_MESH)
    e = np.asarray(sc["ents_pos"][slot], np.float64)
    close = (float(e[0]) - 1.0, 0.0, float(e[2]), 0.0)
    z16 = _render(sc, "PickupObjects", close, CAMERAS[0], 8, 80, 60)
    good = ref.against_frame(ref.label_frame(sc, 80, 60, 8, meshes=golden_meshes(sc), pose=close, cam=CAMERAS[0]), z16)
    bad = ref.against_frame(scaled(sc, close, CAMERAS[0]), z16)
    print(f"PickupObjects mesh: {good} as defined, {bad} scaled after the translation")
    assert good[0] <= MISS_CAP * good[1] and bad[0] > MISS_CAP * bad[1]


def test_bounds_contain_exact_and_the_stats_are_the_codes():
    for cls_name in ("PickupObjects", "Sidewalk", "CollectHealth"):
        sc = _scene(cls_name)
        for k in (0, 3):
            pose = _poses(cls_name, 6)[k]
            exact = _label(sc, cls_name, pose, CAMERAS[0], 8, 80, 60)
            bounds = _label(sc, cls_name, pose, CAMERAS[0], 8, 80, 60, "bounds")
            on_mesh = exact["cls"] == ref.MESH
            assert (bounds["t"][on_mesh] <= exact["t"][on_mesh]).all(), (cls_name, k)
            for label in (exact, bounds):
                E = len(sc["ents_kind"])
                slot = np.where(label["code"] >= ref.RAY_ENT, label["code"] - ref.RAY_ENT, -1)
                assert np.array_equal(label["ent_pixels"], np.bincount(slot[slot >= 0], minlength=E).astype(np.int32))
                for s in range(E):
                    vs, us = np.nonzero(slot == s)
                    want = (us.min(), vs.min(), us.max(), vs.max()) if len(vs) else (80, 60, -1, -1)
                    assert tuple(label["ent_box"][s]) == want, (cls_name, k, s)


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_header_declares_the_entry_point_and_the_build_has_the_units():
    from miniworld_amd import engine
    header = open(os.path.join(ROOT, "include", "mwengine.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", "", header, flags=re.S).split())
    proto = ("int mw_label_frame(mw_engine *e, const mw_label_params *params, const uint8_t *d_mask, uint8_t *d_class, int32_t *d_code, float *d_depth, "
             "int32_t *d_ent_pixels, int32_t *d_ent_box, void *stream);")
    assert proto in text
    assert "struct mw_label_params { double near, far; int32_t flags, pad; }; typedef struct mw_label_params mw_label_params;" in text
    # the binding's mirror of it: the layout mw_label.h asserts of the compiler's
    assert 'static_assert(sizeof(mw_label_params) == 24 && offsetof(mw_label_params, far) == 8 && offsetof(mw_label_params, flags) == 16' in open(
        os.path.join(CSRC, "mw_label.h")).read()
    P = engine.MwLabelParams
    assert C.sizeof(P) == 24 and (P.near.offset, P.far.offset, P.flags.offset, P.pad.offset) == (0, 8, 16, 20) and P.flags.size == 4
    for name, value in (("MW_LABEL_MESH_EXACT", 0), ("MW_LABEL_MESH_BOUNDS", 1), ("MW_LABEL_UNPRUNED", 2)):
        assert re.search(rf"#define {name}\s+{value}\b", header), name
    assert "MW_LABEL_NOTHING = 0, MW_LABEL_FLOOR = 1, MW_LABEL_CEILING = 2, MW_LABEL_WALL = 3, MW_LABEL_FRAME = 4, MW_LABEL_BOX = 5, MW_LABEL_MESH = 6" in text
    assert (engine.LABEL_NOTHING, engine.LABEL_FLOOR, engine.LABEL_CEILING, engine.LABEL_WALL, engine.LABEL_FRAME, engine.LABEL_BOX, engine.LABEL_MESH) == tuple(range(7))
    assert (engine.LABEL_MESH_EXACT, engine.LABEL_MESH_BOUNDS, engine.LABEL_UNPRUNED) == (0, 1, 2)
    assert header.index("---- depth projection") < header.index("---- label frames") < header.index("int mw_label_frame(")
    for cited in ("miniworld.py:1197-1221", "entity.py:150-161", "entity.py:409-432", "miniworld.py:512"):
        assert cited in header, cited
    assert "mw_label_frame" in engine.SIGNATURES and engine.EXPORTS == list(engine.SIGNATURES)
    check_units_built("mw_label.hip", "mw_engine_label.hip")
    check_kernel("mw_label_kernel", "mw_label.hip")
    label_h = open(os.path.join(CSRC, "mw_label.h")).read()
    for shared in ("mwdepth::camera_of", "mwdepth::subpixel_of", "mw::sincos_det"):
        assert shared in label_h, shared
    code = re.sub(r"//[^\n]*", "", label_h)
    for own in ("sin(", "cos(", "tan(", "atan", "fma("):
        assert own not in code.replace("sincos_det(", ""), own
    check_does_not_wait("mw_engine_label.hip")


def test_library_exports_the_entry_point_and_refuses_a_null_engine():
    check_refuses_null_engine("mw_label_frame", None, None, None, None, None, None, None, None)


def test_label_launch(program):
    def launch(*args):
        return launch_of(program, *args, names=("grid", "threads", "lds", "band_rows", "chunk", "fits"))

    def bytes_of(pixels, chunk, ents):
        return (pixels * 10 + chunk * 160 + ents * 92 + 15) // 16 * 16

    # the Hallway at 80 x 60: the whole frame in one band
    l = launch(4096, 80, 60, 8, 1)
    assert l == dict(grid=4096, threads=256, lds=bytes_of(4800, 8, 1), band_rows=60, chunk=8, fits=1)
    # the Maze: polygons in chunks of 64
    l = launch(1024, 80, 60, 700, 1)
    assert (l["chunk"], l["band_rows"], l["lds"], l["fits"]) == (64, 60, bytes_of(4800, 64, 1), 1) and l["lds"] <= 65536
    # 84 x 84 does not fit one band; whatever the size, the bands' bytes stay within 64 KiB and one more row would not
    for W, H, polys, ents in ((84, 84, 64, 8), (160, 120, 300, 21), (320, 240, 8, 1), (4080, 1020, 64, 4), (81, 61, 1, 0), (1, 1, 0, 0)):
        l = launch(8, W, H, polys, ents)
        assert l["fits"] == 1 and 1 <= l["band_rows"] <= H and l["lds"] == bytes_of(l["band_rows"] * W, l["chunk"], ents) <= 65536, (W, H, l)
        assert l["band_rows"] == H or bytes_of((l["band_rows"] + 1) * W, l["chunk"], ents) + 16 > 65536, (W, H, l)
        assert l["chunk"] == max(1, min(polys, 64))
    assert launch(8, 84, 84, 64, 8)["band_rows"] < 84
    # what the engine refuses: a row that does not fit beside the scene, more polygons or slots than a 16-bit code names
    assert launch(8, 6000, 10, 64, 8)["fits"] == 0
    assert launch(8, 80, 60, 0xF001, 1)["fits"] == 0 and launch(8, 80, 60, 0xF000, 1)["fits"] == 1
    assert launch(8, 80, 60, 8, 0x1000)["fits"] == 0
    assert launch(8, 80, 60, 8, 600)["fits"] == 1 and launch(8, 80, 60, 8, 0xFFF)["fits"] == 0         # (4095 slots: 376 740 bytes of volumes)


def test_vec_env_refusals_and_the_recorded_call(monkeypatch):
    import torch
    from miniworld_amd import engine
    from miniworld_amd.vec_env import LabelFrame, MiniWorldVecEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    vec = MiniWorldVecEnv("MiniWorld-PickupObjects-v0", 5)
    E = vec.engine.E
    n0 = len(lib.calls)
    f = vec.label_frame()
    assert len(lib.calls) == n0         # made without the library
    assert isinstance(f, LabelFrame) and (f.meshes, f.near, f.far) == ("exact", 0.04, 100.0)
    assert f.cls.dtype == torch.uint8 and tuple(f.cls.shape) == (5, 60, 80) and f.code.dtype == torch.int32 and tuple(f.code.shape) == (5, 60, 80)
    assert f.depth is None and f.ent_pixels is None and f.ent_box is None
    assert (f.code == -1).all() and (f.slot == -1).all() and f.slot.dtype == torch.int32
    assert vec.label_update(f) is f.cls
    assert [c[0] for c in lib.calls[n0:]] == ["mw_label_frame"]
    args = lib.calls[-1][1]
    p = args[1]._obj
    assert (p.near, p.far, p.flags) == (0.04, 100.0, engine.LABEL_MESH_EXACT) and args[2] is None
    assert args[3].value == f.cls.data_ptr() and args[4].value == f.code.data_ptr() and args[5] is None and args[6] is None and args[7] is None
    # every output, the cylinders, a mask
    g = vec.label_frame(meshes="bounds", depth=True, stats=True, near=0.5, far=20.0)
    assert g.depth.dtype == torch.float32 and tuple(g.depth.shape) == (5, 60, 80) and (g.depth == 20.0).all()
    assert g.ent_pixels.dtype == g.ent_box.dtype == torch.int32 and tuple(g.ent_pixels.shape) == (5, E) and tuple(g.ent_box.shape) == (5, E, 4)
    assert g.ent_box[0, 0].tolist() == [80, 60, -1, -1]
    mask = torch.tensor([1, 0, 0, 1, 1], dtype=torch.uint8)
    vec.label_update(g, mask=mask)
    args = lib.calls[-1][1]
    p = args[1]._obj
    assert (p.near, p.far, p.flags) == (0.5, 20.0, engine.LABEL_MESH_BOUNDS) and args[2].value == mask.data_ptr()
    assert args[5].value == g.depth.data_ptr() and args[6].value == g.ent_pixels.data_ptr() and args[7].value == g.ent_box.data_ptr()
    h = vec.label_frame(code=False)
    assert h.code is None and h.slot is None
    vec.label_update(h)
    assert lib.calls[-1][1][4] is None
    # a slot's view of the code
    g.code[0, 0, 0], g.code[0, 0, 1] = engine.RAY_ENT + 3, 7
    assert g.slot[0, 0, :2].tolist() == [3, -1]
    # refusals
    n0 = len(lib.calls)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(meshes="mesh"), dict(meshes=None), dict(code=1), dict(depth="yes"), dict(stats=None), dict(near=nan), dict(near=-0.1), dict(near=inf),
               dict(far=inf), dict(far=nan), dict(near=2.0, far=2.0), dict(near=3.0, far=2.0), dict(near="a")):
        with pytest.raises(ValueError):
            vec.label_frame(**kw)
    for bad in (None, f.cls, vec.depth_window()):
        with pytest.raises(ValueError):
            vec.label_update(bad)
    for kw in (dict(mask=[1, 0, 0, 1, 0]), dict(mask=mask[:4]), dict(mask=mask.float())):
        with pytest.raises(ValueError):
            vec.label_update(f, **kw)

    def broken(**kw):
        b = LabelFrame(g.cls, g.code, g.depth, g.ent_pixels, g.ent_box, g.meshes, g.near, g.far)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    for b in (broken(cls=None), broken(cls=g.cls[:4]), broken(cls=g.cls.to(torch.int8)), broken(code=g.code.long()), broken(code=g.code[:, :, :79]),
              broken(depth=g.depth.double()), broken(ent_pixels=g.ent_pixels[:, :1]), broken(ent_box=g.ent_box[:, :, :3]), broken(ent_box=g.ent_box.long())):
        with pytest.raises(engine.EngineError):
            vec.label_update(b)
    assert len(lib.calls) == n0         # nothing reached the library


def test_adapter_is_off_by_default_and_reports_the_labels_when_asked(monkeypatch):
    import torch
    from miniworld_amd.vector import MiniWorldVectorEnv
    lib = stub_engine(monkeypatch, {"mw_snapshot_bytes": 4096})
    plain = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2)
    _, info = plain.reset(seed=0)
    _, _, _, _, info2 = plain.step(torch.zeros(2, dtype=torch.int32))
    assert plain.label is None and "label" not in info and "label" not in info2
    assert "mw_label_frame" not in [c[0] for c in lib.calls]
    for bad in (True, 9, [("meshes", "bounds")]):
        with pytest.raises(ValueError):
            MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, label_frame=bad)
    with pytest.raises((ValueError, TypeError)):
        MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, label_frame=dict(mesh="bounds"))
    n0 = len(lib.calls)
    envs = MiniWorldVectorEnv("MiniWorld-Hallway-v0", 2, label_frame=dict(meshes="bounds", stats=True))
    _, info = envs.reset(seed=0)
    assert envs.label.meshes == "bounds" and set(info) == {"label"}
    _, _, _, _, info = envs.step(torch.zeros(2, dtype=torch.int32))
    assert info["label"] is envs.label and info["label"].cls.dtype == torch.uint8 and tuple(info["label"].cls.shape) == (2, 60, 80)
    assert len([c for c in lib.calls[n0:] if c[0] == "mw_label_frame"]) == 2        # one behind the reset, one behind the step
